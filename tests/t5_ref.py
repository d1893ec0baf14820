"""The judge of the T5 encoder tests: an fp64 numpy restatement of transformers' T5EncoderModel (embedding, T5LayerNorm,
bucketed relative-position bias of block 0, masked softmax WITHOUT 1 / sqrt(d), gated gelu_new feed-forward, final norm), written
from the model's definition and independent of ezaudio_amd/t5.py.  `emulate=True` rounds every GEMM / MFMA operand to bf16 where
csrc/t5.hip does (norm output, weights, q / k / v, the un-normalised softmax numerator exp(s - row max), attention output, gated
activation) and keeps everything else in fp64: the spirit of tests/kernel_emul.py -- what the kernels would give with exact
accumulation.  Weights come from oracle.weights.make_tensor with a scale per kind, so nothing depends on an initialiser."""
import numpy as np

from oracle.weights import make_tensor

CONFIGS = {   # both: vocab 97, 32 buckets, max distance 128, head dim 64
    'a': dict(vocab_size=97, d_model=128, d_kv=64, num_heads=2, d_ff=192, num_layers=2),
    'b': dict(vocab_size=97, d_model=192, d_kv=64, num_heads=2, d_ff=256, num_layers=3),   # inner width 128 != d_model 192: a stride taken from the wrong dimension shows
}
for _c in CONFIGS.values():
    _c.update(relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6,
              feed_forward_proj='gated-gelu_new')


def config(name, **over):
    c = dict(CONFIGS[name])
    c.update(over)
    return c


def make_weights(cfg, seed=0):
    """Hugging Face T5EncoderModel state dict (numpy fp32).  Scales: embedding +-1 (T5 embeddings are O(1)); projections xavier, q at 0.35 of it
    (no 1 / sqrt(d) in T5: scores stay O(1 - 10)); norm gains 1 +- 0.1; bias table +-1."""
    D, H, dk, F = cfg['d_model'], cfg['num_heads'], cfg['d_kv'], cfg['d_ff']
    I = H * dk
    sd = {}

    def t(name, shape, kind, mul=1.0):
        sd[name] = (make_tensor('t5.' + name, shape, kind, seed) * np.float32(mul)).astype(np.float32)

    t('shared.weight', (cfg['vocab_size'], D), 'table', 10.0)
    sd['encoder.embed_tokens.weight'] = sd['shared.weight']
    t('encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight', (cfg['relative_attention_num_buckets'], H), 'table', 10.0)
    for n in range(cfg['num_layers']):
        a, f = f'encoder.block.{n}.layer.0', f'encoder.block.{n}.layer.1'
        t(a + '.SelfAttention.q.weight', (I, D), 'xavier', 0.35)
        t(a + '.SelfAttention.k.weight', (I, D), 'xavier')
        t(a + '.SelfAttention.v.weight', (I, D), 'xavier')
        t(a + '.SelfAttention.o.weight', (D, I), 'xavier')
        t(a + '.layer_norm.weight', (D,), 'ln_w')
        t(f + '.DenseReluDense.wi_0.weight', (F, D), 'xavier')
        t(f + '.DenseReluDense.wi_1.weight', (F, D), 'xavier')
        t(f + '.DenseReluDense.wo.weight', (D, F), 'xavier')
        t(f + '.layer_norm.weight', (D,), 'ln_w')
    t('encoder.final_layer_norm.weight', (D,), 'ln_w')
    return sd


def make_ids(cfg, B, L, seed=0):
    from oracle.weights import uniform_pm1
    u = uniform_pm1('t5.ids', B * L, seed).astype(np.float64)
    return np.minimum(((u + 1.0) * 0.5 * cfg['vocab_size']).astype(np.int64), cfg['vocab_size'] - 1).reshape(B, L)


def make_mask(B, L, valid):
    m = np.zeros((B, L), dtype=np.uint8)
    for b, n in enumerate(valid):
        m[b, :n] = 1
    return m


def bf16_round(x):
    """round to nearest even bf16, returned as fp64"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32).astype(np.float64)


def bf16_ulp(x):
    """spacing of bf16 (8 significant bits) at |x| (fp64 array)"""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return 2.0 ** (e - 7)


def bucket(rel, num_buckets=32, max_distance=128):
    """T5's bidirectional bucket of rel = key - query (integer array); the logarithm in float32 as the model computes it."""
    rel = np.asarray(rel, dtype=np.int64)
    nb = num_buckets // 2
    ret = (rel > 0).astype(np.int64) * nb
    n = np.abs(rel)
    max_exact = nb // 2
    with np.errstate(divide='ignore'):
        val = np.log(n.astype(np.float32) / np.float32(max_exact)) / np.float32(np.log(max_distance / max_exact)) * np.float32(nb - max_exact)
    large = max_exact + np.where(n > 0, val, 0).astype(np.int64)
    return ret + np.where(n < max_exact, n, np.minimum(large, nb - 1))


def rms(x, w, eps):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w


def gelu_new(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def attention(q, k, v, bias, mask, emulate=False):
    """q, k, v [B, H, L, d] fp64, bias [H, L(query), L(key)], mask [B, L] -> [B, H, L, d]; masked keys weigh exactly 0"""
    r = bf16_round if emulate else (lambda a: a)
    keep = (np.asarray(mask) != 0)[:, None, None, :]
    kz = np.where(keep.swapaxes(-1, -2), k, 0.0)   # whatever a masked key or value holds (NaN included) is not data
    vz = np.where(keep.swapaxes(-1, -2), v, 0.0)
    s = np.einsum('bhqd,bhkd->bhqk', r(q), r(kz)) + bias[None]
    s = np.where(keep, s, -np.inf)
    p = np.where(keep, np.exp(s - s.max(-1, keepdims=True)), 0.0)
    return np.einsum('bhqk,bhkd->bhqd', r(p), r(vz)) / p.sum(-1, keepdims=True)


def encode(cfg, sd, ids, mask, emulate=False):
    """last_hidden_state [B, L, d_model] in fp64"""
    r = bf16_round if emulate else (lambda a: a)
    W = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    B, L = ids.shape
    H, dk, eps = cfg['num_heads'], cfg['d_kv'], cfg['layer_norm_epsilon']
    x = W['shared.weight'][ids]
    rel = np.arange(L)[None, :] - np.arange(L)[:, None]   # [query, key] = key - query
    tab = W['encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight']
    bias = tab[bucket(rel, cfg['relative_attention_num_buckets'], cfg['relative_attention_max_distance'])].transpose(2, 0, 1)
    heads = lambda t: t.reshape(B, L, H, dk).transpose(0, 2, 1, 3)
    for n in range(cfg['num_layers']):
        a, f = f'encoder.block.{n}.layer.0', f'encoder.block.{n}.layer.1'
        u = r(rms(x, W[a + '.layer_norm.weight'], eps))
        q, k, v = (heads(u @ r(W[a + f'.SelfAttention.{p}.weight']).T) for p in 'qkv')
        o = attention(q, k, v, bias, mask, emulate).transpose(0, 2, 1, 3).reshape(B, L, H * dk)
        x = x + r(o) @ r(W[a + '.SelfAttention.o.weight']).T
        u = r(rms(x, W[f + '.layer_norm.weight'], eps))
        g = gelu_new(u @ r(W[f + '.DenseReluDense.wi_0.weight']).T) * (u @ r(W[f + '.DenseReluDense.wi_1.weight']).T)
        x = x + r(g) @ r(W[f + '.DenseReluDense.wo.weight']).T
    return rms(x, W['encoder.final_layer_norm.weight'], eps)
