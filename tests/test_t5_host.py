"""CPU tests of the T5 encoder's host side: the fp64 judge (tests/t5_ref.py) against transformers, the committed goldens, the bucket
function, the weight packer, the exported ABI and the refusals ezt5_create decides without a GPU."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import t5_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mint():
    spec = importlib.util.spec_from_file_location('mint_t5_golden', os.path.join(ROOT, 'tools', 'mint_t5_golden.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope='module')
def hf_models():
    pytest.importorskip('transformers')
    mint = _mint()
    out = {}
    for name in 'ab':
        cfg = t5_ref.config(name)
        sd = t5_ref.make_weights(cfg, mint.SEED_W)
        out[name] = (cfg, sd, mint.hf_model(cfg, sd))
    return mint, out


@pytest.mark.parametrize('name', ['a', 'b'])
def test_judge_matches_transformers_in_double(hf_models, name):
    """(a) T5EncoderModel in double (T5LayerNorm's float32 variance cast removed: tools/mint_t5_golden.py double_norm -- with the cast the
    'double' model carries ~3e-6 of float32 rounding, measured) against the restatement: 1e-9 max-abs on EVERY position, masks of 1 / 37 / L valid tokens."""
    mint, models = hf_models
    cfg, sd, hf = models[name]
    for L in mint.LENGTHS:
        ids, mask = mint.case_inputs(cfg, L)
        want = mint.run_hf(hf, ids, mask)
        got = t5_ref.encode(cfg, sd, ids, mask)
        err = float(np.abs(got - want).max())
        print(f't5 judge vs transformers {name} L={L}: max-abs {err:.3e}')
        assert np.isfinite(got).all() and err <= 1e-9, (name, L, err)


@pytest.mark.parametrize('name', ['a', 'b'])
def test_goldens_are_what_transformers_gives(hf_models, name):
    """(b) the committed fixtures are the minting script's output (fp32 of the double model) for the inputs the GPU test rebuilds"""
    mint, models = hf_models
    cfg, sd, hf = models[name]
    g = np.load(os.path.join(ROOT, 'tests', 'golden', f't5_tiny_{name}.npz'))
    for L in mint.LENGTHS:
        ids, mask = mint.case_inputs(cfg, L)
        assert np.array_equal(g[f'ids_{L}'], ids) and np.array_equal(g[f'mask_{L}'], mask)
        want = mint.run_hf(hf, ids, mask)
        assert g[f'out_{L}'].dtype == np.float32 and g[f'out_{L}'].shape == (3, L, cfg['d_model'])
        assert np.abs(g[f'out_{L}'].astype(np.float64) - want).max() <= 1e-6 * max(1.0, np.abs(want).max())


def test_goldens_match_the_judge_without_transformers():
    """the same fixtures against the judge alone (fp32 storage: half an fp32 ulp of the largest value)"""
    for name in 'ab':
        g = np.load(os.path.join(ROOT, 'tests', 'golden', f't5_tiny_{name}.npz'))
        cfg = t5_ref.config(name)
        sd = t5_ref.make_weights(cfg, 1)
        for L in (7, 130):
            want = t5_ref.encode(cfg, sd, g[f'ids_{L}'].astype(np.int64), g[f'mask_{L}'])
            assert np.abs(g[f'out_{L}'] - want).max() <= 2.0 ** -24 * np.abs(want).max() + 1e-9
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', f't5_tiny_{name}.npz')) < (1 << 20)


def test_bucket_function_matches_transformers():
    """(c) judge's and product's bucket against T5Attention._relative_position_bucket for key - query in -600 .. 600"""
    M = pytest.importorskip('transformers.models.t5.modeling_t5')
    from ezaudio_amd.t5 import expand_bias_table, relative_position_bucket
    rp = torch.arange(-600, 601)
    for nb, md in ((32, 128), (32, 64), (16, 128)):
        want = M.T5Attention._relative_position_bucket(rp, bidirectional=True, num_buckets=nb, max_distance=md).numpy()
        assert np.array_equal(t5_ref.bucket(rp.numpy(), nb, md), want)
        assert np.array_equal(relative_position_bucket(rp, nb, md).numpy(), want)
    assert want.min() == 0 and want.max() == 15
    tab = torch.arange(32 * 3, dtype=torch.float32).reshape(32, 3)
    e = expand_bias_table(tab, 200, 32, 128)
    assert e.shape == (3, 399)
    d = np.arange(-199, 200)
    assert np.array_equal(e.numpy(), tab.numpy()[t5_ref.bucket(d)].T)


def _create(lib, **over):
    from ezaudio_amd import _lib
    c = dict(vocab=97, d_model=128, d_kv=64, num_heads=2, d_ff=192, num_layers=2, num_buckets=32, max_distance=128, eps=1e-6, max_len=512,
             ff_act=_lib.FF_GATED_GELU_NEW)
    c.update(over)
    h = C.c_void_p()
    rc = lib.ezt5_create(C.byref(_lib.Ezt5Config(*[c[f[0]] for f in _lib.Ezt5Config._fields_])), C.byref(h))
    return rc, h


def test_packer_layout_and_refusals(lib):
    """(d) blob offsets: aligned, disjoint, in table order, every state-dict value where the table says; unknown / missing keys refused"""
    from ezaudio_amd import _lib
    from ezaudio_amd.t5 import T5Encoder
    cfg = t5_ref.config('b')
    sd = {k: torch.tensor(v) for k, v in t5_ref.make_weights(cfg, 1).items()}
    enc = T5Encoder(cfg, device='cpu', max_len=160)
    names = [t['name'] for t in enc.table]
    assert names[:2] == ['embed', 'bias_table'] and names[-1] == 'final_ln' and len(names) == 3 + 6 * cfg['num_layers']
    end = 0
    for t in enc.table:
        assert t['offset'] % 256 == 0 and t['offset'] >= end
        end = t['offset'] + t['rows'] * t['cols'] * (2 if t['dtype'] == _lib.P_BF16 else 4)
    assert end <= enc.blob_bytes < end + 256
    tab = {t['name']: t for t in enc.table}
    D, I, F = cfg['d_model'], cfg['num_heads'] * cfg['d_kv'], cfg['d_ff']
    assert (tab['blk1.wqkv']['rows'], tab['blk1.wqkv']['cols']) == (3 * I, D) and (tab['blk1.wo']['rows'], tab['blk1.wo']['cols']) == (D, I)
    assert (tab['blk2.wi']['rows'], tab['blk2.wi']['cols']) == (2 * F, D) and (tab['blk2.wff']['rows'], tab['blk2.wff']['cols']) == (D, F)
    assert (tab['bias_table']['rows'], tab['bias_table']['cols']) == (cfg['num_heads'], 2 * 160 - 1)
    blob = enc.pack(sd)
    assert blob.numel() == enc.blob_bytes

    def view(name, dtype):
        t = tab[name]
        n = t['rows'] * t['cols'] * (2 if dtype == torch.bfloat16 else 4)
        return blob[t['offset']:t['offset'] + n].view(dtype).reshape(t['rows'], t['cols'])
    a = 'encoder.block.1.layer.0.SelfAttention.'
    assert torch.equal(view('blk1.wqkv', torch.bfloat16), torch.cat([sd[a + 'q.weight'], sd[a + 'k.weight'], sd[a + 'v.weight']]).bfloat16())
    f = 'encoder.block.2.layer.1.DenseReluDense.'
    assert torch.equal(view('blk2.wi', torch.bfloat16), torch.cat([sd[f + 'wi_0.weight'], sd[f + 'wi_1.weight']]).bfloat16())
    assert torch.equal(view('blk2.wff', torch.bfloat16), sd[f + 'wo.weight'].bfloat16())
    assert torch.equal(view('embed', torch.float32), sd['shared.weight'])
    assert torch.equal(view('blk0.ln1', torch.float32)[0], sd['encoder.block.0.layer.1.layer_norm.weight'])
    assert torch.equal(view('final_ln', torch.float32)[0], sd['encoder.final_layer_norm.weight'])
    rb = sd['encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight'].numpy()
    assert np.array_equal(view('bias_table', torch.float32).numpy(), rb[t5_ref.bucket(np.arange(-159, 160))].T)
    # either embedding key alone is enough; both present must agree
    only_shared = {k: v for k, v in sd.items() if k != 'encoder.embed_tokens.weight'}
    assert torch.equal(enc.pack(only_shared), blob)
    with pytest.raises(KeyError, match='unexpected'):
        enc.pack(dict(sd, **{'lm_head.weight': torch.zeros(2, 2)}))
    assert torch.equal(enc.pack(dict(sd, **{'lm_head.weight': torch.zeros(2, 2)}), strict=False), blob)
    with pytest.raises(KeyError, match='missing'):
        enc.pack({k: v for k, v in sd.items() if not k.endswith('block.1.layer.1.DenseReluDense.wi_1.weight')})
    with pytest.raises(KeyError, match='missing'):
        enc.pack({k: v for k, v in sd.items() if k not in ('shared.weight', 'encoder.embed_tokens.weight')})
    with pytest.raises(ValueError):
        enc.pack(dict(sd, **{'encoder.final_layer_norm.weight': torch.zeros(D + 1)}))


def test_library_exports_the_t5_symbols_of_the_header(lib):
    """(e) every ezt5_* function the header declares is exported and bound, and the ABI version did not move"""
    from ezaudio_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ezdit.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(ezt5_[a-z_0-9]+)\s*\(', src))
    assert {'ezt5_create', 'ezt5_destroy', 'ezt5_blob_bytes', 'ezt5_bind_weights', 'ezt5_workspace_bytes', 'ezt5_bind_workspace', 'ezt5_encode',
            'ezt5_test_attention', 'ezt5_test_attention_ex', 'ezt5_test_embed_rms', 'ezt5_test_gated_gelu', 'ezt5_test_gemm'} <= declared
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r' T (ezt5_[a-z_0-9]+)', out))
    assert declared == exported == set(_lib.T5_PROTOTYPES)
    assert lib.ezdit_abi_version() == 4
    body = re.search(r'typedef struct \{([^}]*)\} ezt5_config;', src, flags=re.S).group(1)
    assert re.findall(r'(?:int32_t|float)\s+([a-z_0-9]+);', body) == [f[0] for f in _lib.Ezt5Config._fields_]
    from ezaudio_amd.build import SOURCES
    assert 't5.hip' in SOURCES
    import ezaudio_amd
    assert ezaudio_amd.T5Encoder.__name__ == 'T5Encoder'


def test_create_refuses_what_is_not_built(lib):
    """(f) EZDIT_E_UNSUPPORTED from ezt5_create, no GPU involved"""
    from ezaudio_amd import _lib
    from ezaudio_amd.t5 import T5Encoder
    rc, h = _create(lib)
    assert rc == 0 and h.value
    assert lib.ezt5_workspace_bytes(h, 3, 513) == 0 and b'max_len' in lib.ezdit_last_error()
    assert lib.ezt5_workspace_bytes(h, 3, 100) > 0
    assert lib.ezt5_destroy(h) == 0
    for over, word in ((dict(d_kv=32), b'd_kv'), (dict(d_ff=100), b'd_ff'), (dict(ff_act=_lib.FF_RELU), b'gelu_new'), (dict(ff_act=_lib.FF_GATED_GELU), b'gelu_new'),
                       (dict(d_model=100), b'd_model'), (dict(max_len=513), b'max_len')):
        rc, h = _create(lib, **over)
        assert rc == -2 and not h.value and word in lib.ezdit_last_error(), over
    rc, h = _create(lib, vocab=0)
    assert rc == -1
    with pytest.raises(NotImplementedError, match='gelu_new'):
        T5Encoder(t5_ref.config('a', feed_forward_proj='relu'), device='cpu')
    with pytest.raises(NotImplementedError, match='d_kv'):
        T5Encoder(t5_ref.config('a', d_kv=32), device='cpu')
    with pytest.raises(NotImplementedError, match='d_ff'):
        T5Encoder(t5_ref.config('a', d_ff=100), device='cpu')


def test_native_text_encoder_keyword_defaults_off():
    import inspect
    from ezaudio_amd.api import EzAudio, EzAudio_ControlNet
    for f in (EzAudio.__init__, EzAudio.load_models, EzAudio_ControlNet.__init__):
        assert inspect.signature(f).parameters['native_text_encoder'].default is False


def test_refusals_come_from_the_library_and_to_checks_the_device(lib):
    """ezt5_bind_workspace decides (B, L) before it looks at the buffer, so the binding takes the code of a refused size from the library; to() keeps the
    encoder where it was built and refuses another device"""
    from ezaudio_amd import _lib
    from ezaudio_amd.t5 import T5Encoder
    rc, h = _create(lib, max_len=64)
    assert rc == 0
    assert lib.ezt5_bind_workspace(h, None, 0, 2, 65) == -2 and b'max_len' in lib.ezdit_last_error()
    assert lib.ezt5_bind_workspace(h, None, 0, 0, 8) == -1
    assert lib.ezt5_bind_workspace(h, None, 0, 2, 8) == -1 and b'null workspace' in lib.ezdit_last_error()
    assert lib.ezt5_destroy(h) == 0
    enc = T5Encoder(t5_ref.config('a'), device='cpu', max_len=64)
    with pytest.raises(NotImplementedError, match='max_len'):
        enc._bind(2, 65)
    with pytest.raises(AssertionError):
        enc._bind(0, 8)
    assert enc.to('cpu') is enc and enc.to(torch.device('cpu')) is enc and enc.to(torch.float32) is enc and enc.to(device='cpu') is enc and enc.eval() is enc
    with pytest.raises(_lib.EzditError, match='built on'):
        enc.to('cuda')
    with pytest.raises(_lib.EzditError, match='built on'):
        enc.to(device=torch.device('meta'))
