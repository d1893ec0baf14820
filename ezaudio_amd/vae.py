"""Oobleck VAE (decoder, encoder, bottleneck sampler) on the MI355X path.

Mirrors the reference's call surface:
  * ``OobleckDecoder(**config)``  -- /root/reference/src/modules/stable_vae/models/autoencoders.py:149-190
    (``use_snake=True``, ``final_tanh=False``, ``out_channels=1`` as in ckpts/vae/config.json; anything else raises),
    ``load_state_dict`` takes the reference checkpoint keys (``decoder.layers.N...weight_g / weight_v / bias / alpha / beta``),
    ``__call__(z[B, latent, L]) -> audio[B, 1, L * prod(strides)]``.
  * ``Autoencoder(ckpt_path, model_type='stable_vae', quantization_first=True)`` -- src/modules/autoencoder_wrapper.py:7-83:
    ``ae(embedding=z)`` decodes; ``ae(audio=wav)`` = ``OobleckEncoder`` (autoencoders.py:115-147) + ``VAEBottleneck.encode``
    (models/bottleneck.py:67-87) -> latents for ``editing_audio``.

How it runs: every Conv1d / ConvTranspose1d is one launch of the same bf16 MFMA GEMM that serves the DiT (csrc/gemm.hip) over
token-major activations with zero halo rows (csrc/vae.hip explains the addressing); SnakeBeta is fused with the fp32 -> bf16
cast; residual adds ride in the GEMM epilogue.  weight_norm is folded into the weights once at load time.  The layer
sequence below is host code: it runs once per call (~70 launches), not per denoising step.  No CPU fallback.

Batches ("The batched VAE"): B samples, of one length or ragged, are stacked along the token axis with zero rows between them -- sample b on rows
[b S, b S + len_b) of a level, S one stride per level -- so every conv stays ONE GEMM for the whole batch and a call is ~70 launches, not B x 70.  The gap is at least the
largest halo a conv of the level reads and is derived from the strides; the kernels that write a bf16 operand buffer (csrc/vae.hip, the *_seg forms) WRITE the gap rows as
zero on every launch, they are never assumed zero.  One sample without lengths issues the launches it always issued.
"""
import json
import math
import os

import numpy as np
import torch

from . import _lib


def _fold_weight_norm(g, v):
    """torch.nn.utils.weight_norm (dim 0): w = g * v / ||v||, norm over all dims but the first (nn/layers.py:9-14)."""
    v64 = v.double()
    nrm = v64.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1)))
    return (g.double() * v64 / nrm).float()


def pack_conv_weight(w):
    """Conv1d weight [Co, Ci, K] -> GEMM operand [Co][K * Ci] (tap-major): with token-major activations and `halo` zero rows in
    front, out[l][co] = sum_{tap, ci} x[l + tap * dilation][ci] * W[co][tap * Ci + ci] -- K tile t of the GEMM reads the
    activation rows shifted by (t // (Ci / 64)) * dilation (GemmArgs.conv_*).  A strided conv (k = 2s, stride s) uses the same
    matrix on the buffer viewed as [T / s + 1][s * Ci]."""
    co, ci, k = w.shape
    return w.permute(0, 2, 1).reshape(co, k * ci).contiguous()


def pack_conv_transpose_weight(w, s):
    """ConvTranspose1d weight [Ci, Co, 2s] (stride s, padding ceil(s / 2)) -> GEMM operand [s * Co][2 * Ci]:
    out[q][r * Co + co] = x[q] . w[:, co, r] + x[q - 1] . w[:, co, r + s]; read as [(L + 1) s][Co] and shifted by the padding
    this IS the up-sampled sequence."""
    ci, co, k = w.shape
    assert k == 2 * s
    return w.reshape(ci, co, 2, s).permute(3, 1, 2, 0).reshape(s * co, 2 * ci).contiguous()


DILATIONS = (1, 3, 9)                      # of the three ResidualUnits of a block (autoencoders.py:38-61)
UNIT_HALO = 3 * max(DILATIONS)             # rows a k = 7 conv of dilation d reads beyond the sequence: 3 d


class _Seg:
    """A stacked batch while it runs through the levels: sample b lies on rows [b S, b S + lens[b] * mul // div) of the current level."""

    def __init__(self, lens_dev, B, S):
        self.lens_ptr, self.B, self.S, self.mul, self.div = lens_dev.data_ptr(), B, S, 1, 1


def _check_lengths(lengths, B, width, what, least=1):
    """`lengths` as a list of B ints in [least, width] (ValueError otherwise)."""
    if torch.is_tensor(lengths):
        lengths = lengths.tolist()
    lengths = [int(v) for v in lengths]
    if len(lengths) != B:
        raise ValueError(f'lengths has {len(lengths)} entries for a batch of {B}')
    for v in lengths:
        if v < least or v > width:
            raise ValueError(f'a length of {v} {what}: every sample needs {least} .. {width} (the padded width)')
    return lengths


class _OobleckNet:
    """Buffers, launches and the ResidualUnit shared by decoder and encoder."""

    def _lens_table(self, lengths):
        """The per-sample lengths as ONE int32 device table per call: uploaded on the current stream, no host synchronisation."""
        return torch.tensor(lengths, dtype=torch.int32).to(self.device, non_blocking=True)

    def _group_size(self, S, width, per_row):
        """How many samples of stride S (the last one `width` rows) fit one stacked run while its largest GEMM operand, `per_row` elements per row of the
        first level, stays below what ezvae_gemm addresses."""
        return max(1, (self.max_elems // per_row - 2 * UNIT_HALO - width) // S + 1)

    def _init_common(self, channels, latent_dim, c_mults, strides, device):
        if channels % 64 or latent_dim % 64:
            raise NotImplementedError('channels and latent_dim must be multiples of 64 (GEMM K tile)')
        if any(s % 2 for s in strides):
            raise NotImplementedError('odd strides are not built (output length (L+1)s - 2 ceil(s/2) != L s)')
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.channels, self.latent_dim = channels, latent_dim
        self.c_mults = [1] + list(c_mults)
        self.strides = list(strides)
        self.ratio = int(np.prod(self.strides))
        self.tile = 6      # 128x64 tiles: best of tools/bench_vae.py at 10 s (M up to 120000, N = 128..5120)
        self.max_elems = (1 << 31) - (1 << 20)   # ezvae_gemm refuses operands that reach 2^31 elements: a batch is split into groups that stay below
        self._w = None
        self._bufs = {}

    # ---- weight packing (host, once) -----------------------------------------------------------------------------------
    def _pack_conv(self, sd, used, name, bias=True):
        w = _fold_weight_norm(sd[name + '.weight_g'], sd[name + '.weight_v'])      # [Co, Ci, K]
        used.update({name + '.weight_g', name + '.weight_v'})
        b = None
        if bias:
            b = sd[name + '.bias'].to(self.device)
            used.add(name + '.bias')
        co, ci, k = w.shape
        return dict(w=pack_conv_weight(w).to(self.device, torch.bfloat16), b=b, co=co, ci=ci, k=k)

    def _pack_snake(self, sd, used, name):
        used.update({name + '.alpha', name + '.beta'})
        a = torch.exp(sd[name + '.alpha'])
        ib = 1.0 / (torch.exp(sd[name + '.beta']) + 1e-9)                           # blocks.py:317-318,351-356
        return dict(a=a.to(self.device), ib=ib.to(self.device))

    def _pack_unit(self, sd, used, q):
        return dict(s0=self._pack_snake(sd, used, q + '.0'), c7=self._pack_conv(sd, used, q + '.1'),
                    s1=self._pack_snake(sd, used, q + '.2'), c1=self._pack_conv(sd, used, q + '.3'))

    # ---- buffers -------------------------------------------------------------------------------------------------------
    def _buf(self, tag, rows, cols, dtype):
        """Activation buffer [rows][cols] for role `tag`.  ONE allocation per (tag, width), grown to the longest sequence seen and
        handed out as a view: a long-running process that decodes / encodes many different lengths (`generate_audio(length=...)`,
        `editing_audio` on arbitrary clips) keeps a bounded working set instead of one full buffer set per length (the widths are
        fixed by the architecture, one per level).  Haloed buffers rely on their halo rows being zero and only interiors are
        ever written, so a view with a NEW row count over an old allocation is re-zeroed once, on the current stream (the one
        the kernels run on): stale interior rows would otherwise sit where the new halo is."""
        key = (tag, cols, dtype)
        need = rows * cols
        ent = self._bufs.get(key)
        if ent is None or ent[0].numel() < need:
            ent = [torch.zeros(need, dtype=dtype, device=self.device), rows]
            self._bufs[key] = ent
        elif ent[1] != rows:
            ent[0][:max(need, ent[1] * cols)].zero_()
            ent[1] = rows
        return ent[0][:need].view(rows, cols)

    def release_buffers(self):
        """Drop the cached activation buffers (they are re-created on the next call)."""
        self._bufs = {}

    # ---- launches ------------------------------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f'ezvae call failed ({rc}): {self.lib.ezdit_last_error().decode()}')

    def _snake(self, x_ptr, ldx, sn, out, halo, L, C, st, seg=None, stride_in=None):
        """out[halo + l][:] = bf16(snake(x[l][:])); rows outside [halo, halo + L) are never written (zero).  With `seg` (a stacked batch) the L rows are all
        written: snake inside a sample's interior, zero in the gaps; `stride_in` is the input's sample stride where it differs from the output's."""
        a, ib = (sn['a'].data_ptr(), sn['ib'].data_ptr()) if sn else (None, None)
        o_ptr = out.data_ptr() + halo * out.shape[1] * 2
        if seg is None:
            self._check(self.lib.ezvae_snake_bf16(x_ptr, ldx, a, ib, o_ptr, out.shape[1], L, C, st))
        else:
            self._check(self.lib.ezvae_snake_bf16_seg(x_ptr, ldx, a, ib, o_ptr, out.shape[1], L, C, seg.lens_ptr, seg.B, seg.mul, seg.div,
                                                      seg.S if stride_in is None else stride_in, seg.S, st))

    def _gemm(self, a_ptr, lda, cw, out_ptr, ldo, M, N, K, cpb, tap_bytes, st, resid_ptr=None, ldr=0):
        self._check(self.lib.ezvae_gemm(a_ptr, lda, cw['w'].data_ptr(), K, N, cw['b'].data_ptr() if cw['b'] is not None else None,
                                        resid_ptr, ldr, out_ptr, ldo, M, N, K, cpb, tap_bytes, self.tile, st))

    def _residual_units(self, units, x_ptr, L, C, st, seg=None):
        """three ResidualUnits (autoencoders.py:38-61), dilations 1, 3, 9; returns the pointer of the fp32 [L][C] result"""
        f32, bf16 = torch.float32, torch.bfloat16
        for ui, (unit, d) in enumerate(zip(units, DILATIONS)):
            hb = self._buf(f'h{3 * d}', L + 6 * d, C, bf16)
            self._snake(x_ptr, C, unit['s0'], hb, 3 * d, L, C, st, seg)
            t = self._buf('t', L, C, f32)
            self._gemm(hb.data_ptr(), C, unit['c7'], t.data_ptr(), C, L, C, 7 * C, C // 64, d * C * 2, st)
            tb = self._buf('h0', L, C, bf16)
            self._snake(t.data_ptr(), C, unit['s1'], tb, 0, L, C, st, seg)
            xn = self._buf(f'r{ui & 1}', L, C, f32)
            self._gemm(tb.data_ptr(), C, unit['c1'], xn.data_ptr(), C, L, C, C, 0, 0, st, resid_ptr=x_ptr, ldr=C)
            x_ptr = xn.data_ptr()
        return x_ptr

    def eval(self):
        return self

    def to(self, *a, **k):
        return self


class OobleckDecoder(_OobleckNet):
    """autoencoders.py:149-190"""

    def __init__(self, out_channels=1, channels=128, latent_dim=128, c_mults=(1, 2, 4, 8), strides=(2, 4, 6, 10),
                 use_snake=True, antialias_activation=False, use_nearest_upsample=False, final_tanh=False, device='cuda'):
        if not use_snake or antialias_activation or use_nearest_upsample or final_tanh or out_channels != 1:
            raise NotImplementedError('only the EzAudio VAE recipe is built: snake activations, transposed-conv upsampling, '
                                      'mono output without tanh (ckpts/vae/config.json)')
        self._init_common(channels, latent_dim, c_mults, strides, device)

    def load_state_dict(self, sd, strict=True):
        sd = {(k[len('decoder.'):] if k.startswith('decoder.') else k): torch.as_tensor(v).detach().float().cpu()
              for k, v in sd.items() if not k.startswith(('encoder.', 'bottleneck.'))}
        used = set()

        def conv_t(name, s):
            w = _fold_weight_norm(sd[name + '.weight_g'], sd[name + '.weight_v'])      # [Ci, Co, 2s]
            used.update({name + '.weight_g', name + '.weight_v', name + '.bias'})
            ci, co, k = w.shape
            b = sd[name + '.bias'].repeat(s).to(self.device)
            return dict(w=pack_conv_transpose_weight(w, s).to(self.device, torch.bfloat16), b=b, co=co, ci=ci, s=s)

        n = len(self.strides)
        w = {'conv_in': self._pack_conv(sd, used, 'layers.0'), 'blocks': []}
        for bi in range(n):
            s = self.strides[n - 1 - bi]
            p = f'layers.{1 + bi}.layers'
            w['blocks'].append(dict(snake=self._pack_snake(sd, used, p + '.0'), up=conv_t(p + '.1', s),
                                    units=[self._pack_unit(sd, used, f'{p}.{2 + u}.layers') for u in range(3)]))
        w['snake_out'] = self._pack_snake(sd, used, f'layers.{1 + n}')
        wo = _fold_weight_norm(sd[f'layers.{2 + n}.weight_g'], sd[f'layers.{2 + n}.weight_v'])   # [1, C, 7]
        used.update({f'layers.{2 + n}.weight_g', f'layers.{2 + n}.weight_v'})
        w['conv_out'] = wo[0].t().contiguous().to(self.device)                                     # [7][C] fp32
        if strict and set(sd) - used:
            raise KeyError(f'unexpected keys in VAE decoder state dict: {sorted(set(sd) - used)[:5]}')
        self._w = w
        return self

    def latent_gap(self):
        """Zero rows between two samples at the latent level, so that at EVERY level the gap (it grows with the strides) covers the largest halo a conv of that
        level reads: 3 for the k = 7 convs at both ends, 1 for a transposed conv, 3 x 9 for the residual units after each up-sampling."""
        gap, mul = 3, 1
        for s in reversed(self.strides):
            mul *= s
            gap = max(gap, -(-UNIT_HALO // mul))
        return gap

    def layer_list(self):
        """The decoder's convolutions in forward order, as what decides which inputs an output reads: ('conv', kernel, dilation, padding) for a Conv1d of
        stride 1 and ('up', kernel, stride, padding) for a ConvTranspose1d (autoencoders.py:149-190; the k = 1 convs of the residual units and the
        activations read one position and are left out)."""
        layers = [('conv', 7, 1, 3)]
        for s in reversed(self.strides):
            layers.append(('up', 2 * s, s, math.ceil(s / 2)))
            layers += [('conv', 7, d, 3 * d) for d in DILATIONS]
        return layers + [('conv', 7, 1, 3)]

    def context_frames(self):
        """Half-width of the decoder's receptive field in latent frames, rounded up: the audio of latent frame q -- the samples [q ratio, (q + 1) ratio) -- reads
        no latent frame outside [q - n, q + n].  Walked backwards through layer_list(): the samples [lo, hi] of a level need [lo - p, hi - p + (k - 1) d]
        of the level before through a Conv1d (output t reads t - p + tap d) and [ceil((lo + p - k + 1) / s), floor((hi + p) / s)] through a ConvTranspose1d
        (output t reads input q where 0 <= t + p - q s <= k - 1)."""
        lo, hi = 0, self.ratio - 1
        for kind, k, a, p in reversed(self.layer_list()):
            if kind == 'conv':
                lo, hi = lo - p, hi - p + (k - 1) * a
            else:
                lo, hi = -((k - 1 - p - lo) // a), (hi + p) // a
        return max(-lo, hi)

    def _decode_one(self, zt, out, st, seg=None, Lmax=None):
        """zt fp32 [L][latent] (token-major), out fp32 [L * ratio].  With `seg`: zt [B][Lmax][latent], L the stacked row count (B - 1) S + Lmax, out
        [B][Lmax * ratio]; the same launches over the stacked rows, the segment kernels in place of the plain ones."""
        w = self._w
        lat = zt.shape[-1]
        L = zt.shape[0] if seg is None else (seg.B - 1) * seg.S + Lmax
        f32, bf16 = torch.float32, torch.bfloat16
        # conv_in: k7 pad 3
        xb = self._buf('h3in', L + 6, lat, bf16)
        self._snake(zt.data_ptr(), lat, None, xb, 3, L, lat, st, seg, Lmax)
        c = w['conv_in']
        x = self._buf('x0', L, c['co'], f32)
        self._gemm(xb.data_ptr(), lat, c, x.data_ptr(), c['co'], L, c['co'], 7 * lat, lat // 64, lat * 2, st)
        x_ptr, C = x.data_ptr(), c['co']
        for blk in w['blocks']:
            up = blk['up']
            s, ci, co = up['s'], up['ci'], up['co']
            assert ci == C
            # snake -> [1 | L | 1] halo, transposed conv as one GEMM over (x[q], x[q-1]), q = 0..L
            xb = self._buf('h1', L + 2, ci, bf16)
            self._snake(x_ptr, C, blk['snake'], xb, 1, L, ci, st, seg)
            y = self._buf('up', (L + 1) * s, co, f32)
            self._gemm(xb.data_ptr() + ci * 2, ci, up, y.data_ptr(), s * co, L + 1, s * co, 2 * ci, ci // 64, -ci * 2, st)
            p = math.ceil(s / 2)
            L, C = L * s, co
            x_ptr = y.data_ptr() + p * co * 4                      # rows p .. p + L of the [(L_in+1) s][Co] view
            if seg is not None:                                    # (a sample that began on row b S of the input begins on row b S s of this view)
                seg.S, seg.mul = seg.S * s, seg.mul * s
            x_ptr = self._residual_units(blk['units'], x_ptr, L, C, st, seg)
        xb = self._buf('h3', L + 6, C, bf16)
        self._snake(x_ptr, C, w['snake_out'], xb, 3, L, C, st, seg)
        if seg is None:
            self._check(self.lib.ezvae_conv_out1(xb.data_ptr(), C, w['conv_out'].data_ptr(), out.data_ptr(), L, C, st))
        else:
            self._check(self.lib.ezvae_conv_out1_seg(xb.data_ptr(), C, w['conv_out'].data_ptr(), out.data_ptr(), Lmax * self.ratio, C, seg.lens_ptr, seg.B,
                                                     seg.mul, seg.div, seg.S, st))

    @torch.no_grad()
    def __call__(self, z, lengths=None):
        """z [B, latent, Lmax] -> audio [B, 1, Lmax * ratio].  `lengths` (B latent lengths, each 1 .. Lmax): sample b is decoded as z[b, :, :lengths[b]] alone is
        -- what lies behind is never read and may be NaN -- and its audio is exactly zero beyond lengths[b] * ratio.  The batch runs as ONE layer sequence over
        the stacked samples (~70 launches, not B x 70); B > 1 without lengths is that path with all lengths equal.  One sample without lengths issues the
        launches it always issued, argument for argument: the same bits, no length table, no gap."""
        if self._w is None:
            raise RuntimeError('load_state_dict() first')
        z = torch.as_tensor(z).to(self.device, torch.float32)
        if z.dim() != 3 or z.shape[1] != self.latent_dim:
            raise ValueError(f'expected latents [B, {self.latent_dim}, L], got {tuple(z.shape)}')
        B, _, L = z.shape
        if lengths is not None:
            lengths = _check_lengths(lengths, B, L, 'cannot be decoded')
        st = torch.cuda.current_stream(self.device).cuda_stream
        if B == 1:                                                 # one sample has no neighbour: today's launches, on its own frames
            n = L if lengths is None else lengths[0]
            zt = z[:, :, :n].transpose(1, 2).contiguous()
            out = (torch.empty if n == L else torch.zeros)(1, 1, L * self.ratio, dtype=torch.float32, device=self.device)
            self._decode_one(zt[0], out[0, 0, :n * self.ratio], st)
            return out
        zt = z.transpose(1, 2).contiguous()
        out = torch.empty(B, 1, L * self.ratio, dtype=torch.float32, device=self.device)
        lens = self._lens_table(lengths if lengths is not None else [L] * B)
        S = L + self.latent_gap()
        ch = self.channels
        widths = [max(self.latent_dim, self.c_mults[-1] * ch)]     # elements per latent row of the widest operand of each level
        mul = 1
        for i in range(len(self.strides), 0, -1):
            mul *= self.strides[i - 1]
            widths.append(mul * self.c_mults[i - 1] * ch)
        n = self._group_size(S, L, max(widths))
        for g in range(0, B, n):
            e = min(B, g + n)
            self._decode_one(zt[g:e], out[g:e], st, _Seg(lens[g:e], e - g, S), L)
        return out

    forward = __call__

    def flops(self, L):
        ch = self.channels
        cm = self.c_mults
        f = 2 * L * cm[-1] * ch * self.latent_dim * 7
        for i in range(len(cm) - 1, 0, -1):
            ci, co, s = cm[i] * ch, cm[i - 1] * ch, self.strides[i - 1]
            f += 2 * L * ci * co * 2 * s
            L *= s
            f += 3 * 2 * L * co * co * 8
        return f + 2 * L * ch * 7


class OobleckEncoder(_OobleckNet):
    """autoencoders.py:115-147.  ``latent_dim`` is the encoder's output width (2 x the VAE latent: mean | scale).

    ``__call__(wav[B, 1, T]) -> [B, latent_dim, T // prod(strides)]`` (reference layout).  A strided WNConv1d (k = 2s, stride s,
    padding s/2) is a plain GEMM: with s/2 zero halo rows in front, output row q reads the 2 s Ci contiguous values that start
    at token q s -- the activation buffer viewed as [T/s + 1][s Ci] with K = 2 s Ci spanning two view rows.
    """

    def __init__(self, in_channels=1, channels=128, latent_dim=256, c_mults=(1, 2, 4, 8), strides=(2, 4, 6, 10),
                 use_snake=True, antialias_activation=False, device='cuda'):
        if not use_snake or antialias_activation or in_channels != 1:
            raise NotImplementedError('only the EzAudio VAE recipe is built: mono input, snake activations')
        self._init_common(channels, latent_dim, c_mults, strides, device)

    def load_state_dict(self, sd, strict=True):
        sd = {(k[len('encoder.'):] if k.startswith('encoder.') else k): torch.as_tensor(v).detach().float().cpu()
              for k, v in sd.items() if not k.startswith(('decoder.', 'bottleneck.'))}
        used = set()
        n = len(self.strides)
        wi = _fold_weight_norm(sd['layers.0.weight_g'], sd['layers.0.weight_v'])                   # [C, 1, 7]
        used.update({'layers.0.weight_g', 'layers.0.weight_v', 'layers.0.bias'})
        w = {'conv_in': dict(w=wi[:, 0].t().contiguous().to(self.device), b=sd['layers.0.bias'].to(self.device)), 'blocks': []}
        for bi in range(n):
            p = f'layers.{1 + bi}.layers'
            w['blocks'].append(dict(units=[self._pack_unit(sd, used, f'{p}.{u}.layers') for u in range(3)],
                                    snake=self._pack_snake(sd, used, p + '.3'), down=self._pack_conv(sd, used, p + '.4'),
                                    s=self.strides[bi]))
        w['snake_out'] = self._pack_snake(sd, used, f'layers.{1 + n}')
        w['conv_out'] = self._pack_conv(sd, used, f'layers.{2 + n}')
        if strict and set(sd) - used:
            raise KeyError(f'unexpected keys in VAE encoder state dict: {sorted(set(sd) - used)[:5]}')
        self._w = w
        return self

    def latent_lengths(self, lengths):
        """Latent frames of clips of `lengths` samples: the chain of floors of the strided convs is one floor by their product."""
        return [int(v) // self.ratio for v in lengths]

    def sample_stride(self, Tmax):
        """Rows per sample at the waveform level: Tmax plus a gap that, divided by the strides so far, still covers the largest halo a conv of every level
        reads (3 x 9 for the residual units, s / 2 for the strided conv behind them, 1 for the k = 3 output conv), rounded up to a multiple of the stride
        product so that every level's stride is an integer."""
        gap, div = 0, 1
        for s in self.strides:
            gap = max(gap, max(UNIT_HALO, s // 2) * div)
            div *= s
        gap = max(gap, div)
        return -(-(Tmax + gap) // self.ratio) * self.ratio

    def _encode_one(self, wav, st, seg=None, Tmax=None):
        """wav fp32 [T] -> fp32 [L][latent_dim] token-major (a cached buffer).  With `seg`: wav [B][Tmax], the result stacked with seg.S rows per sample
        (what lies in the gaps is not meaningful)."""
        w = self._w
        T = wav.shape[0] if seg is None else (seg.B - 1) * seg.S + Tmax
        f32, bf16 = torch.float32, torch.bfloat16
        C = self.channels
        x = self._buf('x0', T, C, f32)
        if seg is None:
            self._check(self.lib.ezvae_conv_in1(wav.data_ptr(), w['conv_in']['w'].data_ptr(), w['conv_in']['b'].data_ptr(),
                                                x.data_ptr(), T, C, st))
        else:
            self._check(self.lib.ezvae_conv_in1_seg(wav.data_ptr(), w['conv_in']['w'].data_ptr(), w['conv_in']['b'].data_ptr(), x.data_ptr(), T, C,
                                                    seg.lens_ptr, seg.B, Tmax, seg.S, st))
        x_ptr, L = x.data_ptr(), T
        for blk in w['blocks']:
            s, dn = blk['s'], blk['down']
            assert dn['ci'] == C and dn['k'] == 2 * s
            x_ptr = self._residual_units(blk['units'], x_ptr, L, C, st, seg)
            p = s // 2
            xb = self._buf(f'h{p}', L + 2 * p, C, bf16)
            self._snake(x_ptr, C, blk['snake'], xb, p, L, C, st, seg)
            Lo = L // s                                              # floor((L + 2p - 2s) / s) + 1 for even s
            if Lo < 1:
                raise ValueError('audio too short for the encoder strides')
            y = self._buf('dn', Lo, dn['co'], f32)
            self._gemm(xb.data_ptr(), s * C, dn, y.data_ptr(), dn['co'], Lo, dn['co'], 2 * s * C, 0, 0, st)
            x_ptr, L, C = y.data_ptr(), Lo, dn['co']
            if seg is not None:                                      # (the stride is a multiple of s: sample b's rows begin at b S / s)
                seg.S, seg.div = seg.S // s, seg.div * s
        xb = self._buf('h1', L + 2, C, bf16)
        self._snake(x_ptr, C, w['snake_out'], xb, 1, L, C, st, seg)
        co = w['conv_out']
        out = self._buf('out', L, co['co'], f32)
        self._gemm(xb.data_ptr(), C, co, out.data_ptr(), co['co'], L, co['co'], 3 * C, C // 64, C * 2, st)
        return out

    @torch.no_grad()
    def __call__(self, audio, lengths=None):
        """audio [B, 1, Tmax] -> [B, latent_dim, Tmax // ratio].  `lengths` (B lengths in samples, each at least the stride product and at most Tmax): sample b
        is encoded as audio[b, :, :lengths[b]] alone is -- what lies behind is never read and may be NaN; the result is [B, latent_dim, max_b(lengths[b] // ratio)],
        exactly zero beyond each sample's own latent length (`latent_lengths`).  The batch runs as ONE layer sequence over the stacked samples; B > 1 without
        lengths is that path with all lengths equal.  One sample without lengths issues the launches it always issued, argument for argument: the same bits,
        no length table, no gap."""
        if self._w is None:
            raise RuntimeError('load_state_dict() first')
        audio = torch.as_tensor(audio).to(self.device, torch.float32).contiguous()
        if audio.dim() != 3 or audio.shape[1] != 1:
            raise ValueError(f'expected audio [B, 1, T], got {tuple(audio.shape)}')
        B, _, T = audio.shape
        if lengths is not None:
            lengths = _check_lengths(lengths, B, T, 'cannot be encoded', least=self.ratio)
        st = torch.cuda.current_stream(self.device).cuda_stream
        if B == 1:                                                   # one sample has no neighbour: today's launches, on its own samples
            wav = audio[0, 0] if lengths is None else audio[0, 0, :lengths[0]]
            return torch.stack([self._encode_one(wav, st).t().clone()])
        if T < self.ratio:
            raise ValueError('audio too short for the encoder strides')
        lens = self._lens_table(lengths if lengths is not None else [T] * B)
        lat_len = torch.div(lens, self.ratio, rounding_mode='floor')
        Lmax = (max(lengths) if lengths is not None else T) // self.ratio
        S = self.sample_stride(T)
        Sn = S // self.ratio
        cn = self.latent_dim
        result = torch.empty(B, cn, Lmax, dtype=torch.float32, device=self.device)
        ch, div, per_row = self.channels, 1, self.channels
        for i, s in enumerate(self.strides):                         # elements per waveform row of the widest operand: level i is C_i wide, 1 / div rows
            per_row = max(per_row, -(-self.c_mults[i] * ch // div))
            div *= s
        n = self._group_size(S, T, per_row)
        for g in range(0, B, n):
            e = min(B, g + n)
            out = self._encode_one(audio[g:e, 0], st, _Seg(lens[g:e], e - g, S), T)
            rows = out.as_strided((e - g, Lmax, cn), (Sn * cn, cn, 1))        # sample b's frames: rows b Sn .. of the stacked result
            keep = (torch.arange(Lmax, device=self.device)[None, :] < lat_len[g:e, None])[:, None, :]
            result[g:e] = torch.where(keep, rows.transpose(1, 2), torch.zeros((), dtype=torch.float32, device=self.device))
        return result

    forward = __call__


def draw_bottleneck_noise(latent, lengths, width, device):
    """The bottleneck noise of a ragged batch, [B, latent, width] and zero beyond each sample's length: one randn(1, latent, lengths[b]) per sample from the
    global generator, in batch order -- exactly the draws B single encodes in that order make (ONE randn(B, latent, width) would change every sample's numbers)."""
    noise = torch.zeros(len(lengths), latent, width, device=device, dtype=torch.float32)
    for b, n in enumerate(lengths):
        noise[b:b + 1, :, :n] = torch.randn(1, latent, n, device=device, dtype=torch.float32)
    return noise


class VAEBottleneck:
    """models/bottleneck.py:73-90: encode = split (mean | scale), sample; decode = identity."""

    def __init__(self, device='cuda'):
        self.lib = _lib.load()
        self.device = torch.device(device)

    def encode(self, x, return_info=False, noise=None, lengths=None, **kwargs):
        """x [B, 2 latent, L] (mean | scale) -> z [B, latent, L].  `lengths` (B latent lengths, each 1 .. L): z is sampled on each sample's own frames -- what lies
        behind is never read and may be NaN -- and is exactly zero beyond; without `noise` every sample draws its own randn(1, latent, lengths[b]) from the
        global generator, in batch order: the numbers that B single calls in that order draw.  A batch is one launch; one sample without lengths issues the
        launch it always issued."""
        if return_info:
            raise NotImplementedError('the KL term is a training quantity')
        x = torch.as_tensor(x).to(self.device, torch.float32)
        B, C2, L = x.shape
        lat = C2 // 2
        if lengths is not None:
            lengths = _check_lengths(lengths, B, L, 'cannot be sampled')
        if noise is None:
            if lengths is None:
                noise = torch.randn(B, lat, L, device=self.device, dtype=torch.float32)    # torch.randn_like(mean), bottleneck.py:69
            else:
                noise = draw_bottleneck_noise(lat, lengths, L, self.device)
        elif lengths is not None and tuple(noise.shape) != (B, lat, L):
            raise ValueError(f'expected noise [{B}, {lat}, {L}] (padded), got {tuple(noise.shape)}')
        noise = torch.as_tensor(noise).to(self.device, torch.float32).contiguous()
        xt = x.transpose(1, 2).contiguous()
        z = torch.empty(B, lat, L, device=self.device, dtype=torch.float32)
        st = torch.cuda.current_stream(self.device).cuda_stream
        if B == 1 and (lengths is None or lengths[0] == L):
            rc = self.lib.ezvae_sample(xt[0].data_ptr(), noise[0].data_ptr(), z[0].data_ptr(), L, lat, st)
        else:
            lens = torch.tensor(lengths if lengths is not None else [L] * B, dtype=torch.int32).to(self.device, non_blocking=True)
            rc = self.lib.ezvae_sample_seg(xt.data_ptr(), noise.data_ptr(), z.data_ptr(), L, lat, lens.data_ptr(), B, 1, 1, L, st)
        if rc != 0:
            raise RuntimeError(f'ezvae_sample failed ({rc}): {self.lib.ezdit_last_error().decode()}')
        return z

    def decode(self, x):
        return x


class _AE:
    """``Autoencoder.ae`` of the reference (an AudioAutoencoder): only the pieces the inference path touches."""

    def __init__(self, encoder, decoder, bottleneck):
        self.encoder = encoder
        self.decoder = decoder
        self.bottleneck = bottleneck


class Autoencoder:
    """src/modules/autoencoder_wrapper.py:7-83 for model_type='stable_vae' (the only type EzAudio's configs use)."""

    def __init__(self, ckpt_path=None, model_type='stable_vae', quantization_first=True, device='cuda', config=None, state_dict=None):
        if model_type != 'stable_vae':
            raise NotImplementedError(f'Model type not implemented: {model_type}')
        if not quantization_first:
            raise NotImplementedError('quantization_first=False decodes through the VAE bottleneck sampler; EzAudio uses True '
                                      '(api/ezaudio.py:76-78)')
        if config is None:
            with open(os.path.join(os.path.dirname(ckpt_path), 'config.json')) as f:     # stable_vae/__init__.py:14-19
                config = json.load(f)
        dec = config['model']['decoder']
        if dec['type'] != 'oobleck':
            raise NotImplementedError(f"decoder type {dec['type']}")
        self.config = config
        decoder = OobleckDecoder(device=device, **dec['config'])
        if state_dict is None:
            sd = torch.load(ckpt_path, map_location='cpu')['state_dict']                 # stable_vae/__init__.py:25-28
            state_dict = {k[len('autoencoder.'):]: v for k, v in sd.items() if k.startswith('autoencoder.')}
        decoder.load_state_dict({k: v for k, v in state_dict.items() if k.startswith('decoder.')})
        encoder = None
        enc = config['model'].get('encoder')
        if enc is not None and any(k.startswith('encoder.') for k in state_dict):
            if enc['type'] != 'oobleck' or config['model'].get('bottleneck', {}).get('type') != 'vae':
                raise NotImplementedError(f"encoder type {enc['type']} / bottleneck {config['model'].get('bottleneck')}")
            encoder = OobleckEncoder(device=device, **enc['config'])
            encoder.load_state_dict({k: v for k, v in state_dict.items() if k.startswith('encoder.')})
        self.ae = _AE(encoder, decoder, VAEBottleneck(device))
        self.model_type = model_type
        self.quantization_first = quantization_first

    def __call__(self, audio=None, embedding=None, lengths=None):
        """`lengths` (one per sample; samples for `audio`, latent frames for `embedding`) makes the call a ragged batch: every sample is encoded / decoded as it
        alone is, the result padded with zeros (OobleckEncoder / OobleckDecoder).  Without it the call is what it always was."""
        if audio is not None:                                                            # autoencoder_wrapper.py:69-73
            if self.ae.encoder is None:
                raise RuntimeError('this Autoencoder was loaded without encoder weights')
            if lengths is None:
                return self.ae.bottleneck.encode(self.ae.encoder(audio))
            enc = self.ae.encoder(audio, lengths=lengths)
            return self.ae.bottleneck.encode(enc, lengths=self.ae.encoder.latent_lengths(lengths))
        if embedding is not None:
            return self.ae.decoder(embedding) if lengths is None else self.ae.decoder(embedding, lengths=lengths)
        raise ValueError('Either audio or embedding must be provided.')

    forward = __call__

    def latent_lengths(self, lengths):
        """Latent frames that clips of `lengths` samples encode to (what ``self(audio=..., lengths=lengths)`` is valid on, per sample)."""
        if self.ae.encoder is None:
            raise RuntimeError('this Autoencoder was loaded without encoder weights')
        return self.ae.encoder.latent_lengths(lengths)

    def decoder_context_frames(self):
        """Half-width of the decoder's receptive field in latent frames (OobleckDecoder.context_frames, computed from its layer list): the context that
        sampler.decode_circular wraps around a ring of latents so that the decode equals one with circular convolutions."""
        return self.ae.decoder.context_frames()

    def eval(self):
        return self

    def to(self, *a, **k):
        return self
