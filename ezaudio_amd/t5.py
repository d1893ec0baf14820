"""T5 text encoder on the MI355X path: stands in for ``transformers.T5EncoderModel`` in the ``text_encoder`` slot.

    enc = T5Encoder.from_hf(hf_model, device)          # or T5Encoder(config, device); enc.load_state_dict(sd)
    ctx = enc(input_ids=ids, attention_mask=mask).last_hidden_state     # fp32 [B, L, d_model], on the device

which is all ``sampler.inference`` reads, so ``EzAudio(..., text_encoder=enc)`` and ``inference(..., text_encoder=enc)`` take it as
they are.  Encoder stacks of the flan-t5 / T5 v1.1 family: gated ``gelu_new`` feed-forward, head dim 64 (anything else raises
NotImplementedError from ``ezt5_create``).  The tokenizer stays with ``transformers``.

The layer sequence is in csrc/t5.hip (``ezt5_encode``: seven launches per layer, projections on the DiT's bf16 MFMA GEMM, fp32
residual stream).  This module packs the weights (one device blob laid out by ``ezt5_blob_bytes``), expands the relative-position
bias of block 0 into the ``[heads][2 max_len - 1]`` table the attention kernel reads, and caches one workspace per (B, L).
No CPU fallback.
"""
import ctypes as C
import math
from types import SimpleNamespace

import torch

from . import _lib

_FF = {'gated-gelu_new': _lib.FF_GATED_GELU_NEW, 'gated-gelu': _lib.FF_GATED_GELU, 'relu': _lib.FF_RELU}


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """transformers' ``T5Attention._relative_position_bucket`` with ``bidirectional=True``, operation for operation (float32 log),
    on an integer tensor of ``key - query`` distances."""
    rp = torch.as_tensor(relative_position, dtype=torch.long)
    nb = num_buckets // 2
    buckets = (rp > 0).to(torch.long) * nb
    rp = torch.abs(rp)
    max_exact = nb // 2
    is_small = rp < max_exact
    large = max_exact + (torch.log(rp.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return buckets + torch.where(is_small, rp, large)


def expand_bias_table(rel_bias, max_len, num_buckets, max_distance):
    """relative_attention_bias.weight [num_buckets, heads] -> [heads, 2 max_len - 1]: entry (key - query) + max_len - 1."""
    d = torch.arange(-(max_len - 1), max_len)
    return rel_bias.float()[relative_position_bucket(d, num_buckets, max_distance)].t().contiguous()


def _cfg_dict(config):
    if isinstance(config, dict):
        return dict(config)
    return config.to_dict() if hasattr(config, 'to_dict') else dict(vars(config))


class T5Encoder:
    def __init__(self, config, device='cuda', max_len=512):
        c = _cfg_dict(config)
        self.lib = _lib.load()
        self.device = torch.device(device)
        ff = c.get('feed_forward_proj', 'relu')
        self.cfg = dict(vocab=int(c['vocab_size']), d_model=int(c['d_model']), d_kv=int(c['d_kv']), num_heads=int(c['num_heads']),
                        d_ff=int(c['d_ff']), num_layers=int(c['num_layers']),
                        num_buckets=int(c.get('relative_attention_num_buckets', 32)),
                        max_distance=int(c.get('relative_attention_max_distance', 128)),
                        eps=float(c.get('layer_norm_epsilon', 1e-6)), max_len=int(max_len), ff_act=_FF.get(ff, _lib.FF_OTHER))
        self._h = C.c_void_p()
        cc = _lib.Ezt5Config(*[self.cfg[f[0]] for f in _lib.Ezt5Config._fields_])
        _lib.check(self.lib.ezt5_create(C.byref(cc), C.byref(self._h)))
        n = self.lib.ezt5_tensor_count(self._h)
        tab = (_lib.Ezt5TensorInfo * n)()
        self.blob_bytes = self.lib.ezt5_blob_bytes(self._h, tab, n)
        self.table = [dict(name=t.name.decode(), dtype=t.dtype, rows=t.rows, cols=t.cols, offset=t.offset) for t in tab]
        self._blob = None
        self._ws = {}       # (B, L) -> workspace tensor
        self._bound = None

    def __del__(self):
        try:
            if self._h:
                self.lib.ezt5_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    # ---- weights ---------------------------------------------------------------------------------------------------------
    def _sources(self):
        """slot name -> list of state-dict keys stacked along dim 0 (bias_table: the key it is expanded from)"""
        src = {'final_ln': ['encoder.final_layer_norm.weight'],
               'bias_table': ['encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight']}
        for n in range(self.cfg['num_layers']):
            a, f = f'encoder.block.{n}.layer.0', f'encoder.block.{n}.layer.1'
            src[f'blk{n}.ln0'] = [a + '.layer_norm.weight']
            src[f'blk{n}.wqkv'] = [a + f'.SelfAttention.{p}.weight' for p in 'qkv']
            src[f'blk{n}.wo'] = [a + '.SelfAttention.o.weight']
            src[f'blk{n}.ln1'] = [f + '.layer_norm.weight']
            src[f'blk{n}.wi'] = [f + '.DenseReluDense.wi_0.weight', f + '.DenseReluDense.wi_1.weight']
            src[f'blk{n}.wff'] = [f + '.DenseReluDense.wo.weight']
        return src

    def pack(self, sd, strict=True):
        """Hugging Face ``T5EncoderModel`` state dict -> the weight blob (uint8 CPU tensor of ``blob_bytes``)."""
        sd = {k: v.detach().cpu() for k, v in sd.items()}
        emb_keys = [k for k in ('shared.weight', 'encoder.embed_tokens.weight') if k in sd]
        if not emb_keys:
            raise KeyError('missing key: shared.weight (or encoder.embed_tokens.weight)')
        if len(emb_keys) == 2 and not torch.equal(sd[emb_keys[0]], sd[emb_keys[1]]):
            raise ValueError('shared.weight and encoder.embed_tokens.weight differ')
        src = self._sources()
        used = set(emb_keys)
        blob = torch.zeros(self.blob_bytes, dtype=torch.uint8)
        for t in self.table:
            name = t['name']
            keys = emb_keys[:1] if name == 'embed' else src[name]
            missing = [k for k in keys if k not in sd]
            if missing:
                raise KeyError(f'missing key(s): {missing}')
            used.update(keys)
            w = torch.cat([sd[k].float().reshape(sd[k].shape[0], -1) if sd[k].dim() > 1 else sd[k].float().reshape(1, -1) for k in keys], 0)
            if name == 'bias_table':
                if tuple(w.shape) != (self.cfg['num_buckets'], self.cfg['num_heads']):
                    raise ValueError(f'{keys[0]}: shape {tuple(w.shape)}, expected {(self.cfg["num_buckets"], self.cfg["num_heads"])}')
                w = expand_bias_table(w, self.cfg['max_len'], self.cfg['num_buckets'], self.cfg['max_distance'])
            if tuple(w.shape) != (t['rows'], t['cols']):
                raise ValueError(f'{name} <- {keys}: shape {tuple(w.shape)}, expected {(t["rows"], t["cols"])}')
            w = w.contiguous().to(torch.bfloat16 if t['dtype'] == _lib.P_BF16 else torch.float32)
            raw = w.view(torch.uint8).reshape(-1)
            blob[t['offset']:t['offset'] + raw.numel()] = raw
        if strict:
            extra = sorted(k for k in sd if k not in used)
            if extra:
                raise KeyError(f'unexpected key(s): {extra[:8]}')
        return blob

    def load_state_dict(self, sd, strict=True):
        blob = self.pack(sd, strict=strict).to(self.device)
        _lib.check(self.lib.ezt5_bind_weights(self._h, blob.data_ptr(), blob.numel()))
        self._blob = blob
        return self

    @classmethod
    def from_hf(cls, hf_model, device='cuda', max_len=512):
        enc = cls(hf_model.config, device, max_len=max_len)
        return enc.load_state_dict(hf_model.state_dict())

    def eval(self):
        return self

    def to(self, *a, **k):
        """Accepted for the slot's sake (``text_encoder.to(device)``).  The weights live where the encoder was built: another device raises, a dtype is
        ignored (the blob's formats are fixed)."""
        dev = k.get('device')
        for x in a:
            if isinstance(x, (str, torch.device)):
                dev = x
            elif isinstance(x, torch.Tensor):
                dev = x.device
        if dev is not None:
            dev = torch.device(dev)
            same = dev.type == self.device.type and (dev.index is None or self.device.index is None or dev.index == self.device.index)
            if not same:
                raise _lib.EzditError(f'T5Encoder.to({dev}): the encoder was built on {self.device}; build another one there (from_hf / load_state_dict)')
        return self

    # ---- forward ---------------------------------------------------------------------------------------------------------
    def _bind(self, B, L):
        if self._bound == (B, L):
            return
        ws = self._ws.get((B, L))
        if ws is None:
            n = self.lib.ezt5_workspace_bytes(self._h, B, L)
            if n == 0:   # refused: ezt5_bind_workspace decides the same thing first and returns the code
                _lib.check(self.lib.ezt5_bind_workspace(self._h, None, 0, B, L))
                raise _lib.EzditError(f'ezt5_workspace_bytes: 0 bytes for B={B} L={L}')
            ws = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._ws[(B, L)] = ws
        _lib.check(self.lib.ezt5_bind_workspace(self._h, ws.data_ptr(), ws.numel(), B, L))
        self._bound = (B, L)

    def __call__(self, input_ids=None, attention_mask=None, **_):
        if self._blob is None:
            raise _lib.EzditError('T5Encoder: load_state_dict has not been called')
        ids = input_ids.to(self.device, torch.int32).contiguous()
        B, L = ids.shape
        mask = torch.ones(B, L, dtype=torch.uint8, device=self.device) if attention_mask is None else \
            attention_mask.to(self.device).ne(0).to(torch.uint8).contiguous()
        self._bind(B, L)
        out = torch.empty(B, L, self.cfg['d_model'], dtype=torch.float32, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self.lib.ezt5_encode(self._h, ids.data_ptr(), mask.data_ptr(), out.data_ptr(), B, L, st))
        return SimpleNamespace(last_hidden_state=out)
