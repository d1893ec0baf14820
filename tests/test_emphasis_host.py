"""Prompt emphasis on the host (no GPU): the '(words:1.6)' parser, the alignment of character spans with tokens through tokenizers that give no offsets, and the exports."""
import pytest

from ezaudio_amd import sampler as S
from ezaudio_amd.sampler import LatentSampler as _RealSampler    # (bound at collection: an earlier test module replaces the module attribute for good)


class WordTok:
    """one token per word (its hash), EOS with add_special_tokens"""
    pieces = 1

    def __call__(self, text, add_special_tokens=True, **kw):
        ids = [1000 + 7 * sum(map(ord, w)) % 900 + 10 * k for w in text.split() for k in range(self.pieces)]
        return type('Enc', (), dict(input_ids=ids + ([1] if add_special_tokens else [])))()


class PieceTok(WordTok):
    """every word in two pieces"""
    pieces = 2


def test_groups_nest_and_multiply():
    assert S.parse_emphasis('(a dog barking:1.6) in (light rain:0.7)') == ('a dog barking in light rain', [(0, 13, 1.6), (17, 27, 0.7)])
    clean, spans = S.parse_emphasis('a (b (c:2) d:1.5) e')
    assert clean == 'a b c d e' and spans == [(2, 7, 1.5), (4, 5, 3.0)]


def test_escapes_and_plain_parentheses_are_text():
    assert S.parse_emphasis(r'x \(y\) (z:2)') == ('x (y) z', [(6, 7, 2.0)])
    assert S.parse_emphasis('a (plain) b') == ('a (plain) b', [])
    assert S.parse_emphasis('no markup here') == ('no markup here', [])


def test_weight_zero_removes_the_group():
    assert S.parse_emphasis('a (b:0) c') == ('a c', [])
    assert S.parse_emphasis('(a:0) (b:2)') == ('b', [(0, 1, 2.0)])
    assert S.parse_emphasis('a (b (c:0) d:2) e') == ('a b d e', [(2, 5, 2.0)])


@pytest.mark.parametrize('text', ['x y:2) z', '(a:5000)', '(a:0.0001)', '((a:64):64)'])
def test_unbalanced_markup_and_weights_out_of_range_raise(text):
    with pytest.raises(ValueError):
        S.parse_emphasis(text)


@pytest.mark.parametrize('tok,per', [(WordTok(), 1), (PieceTok(), 2)])
def test_spans_map_to_tokens_without_offsets(tok, per):
    clean, spans = S.parse_emphasis('a (b (c:2) d:1.5) e')
    w = S.emphasis_weights(tok, clean, spans, 16)
    word = [1.0, 1.5, 3.0, 1.5, 1.0]
    assert w == [x for x in word for _ in range(per)] + [1.0] * (16 - 5 * per)      # EOS and the padding weigh 1
    assert S.emphasis_weights(tok, 'plain words only', [], 8) == [1.0] * 8
    # truncation truncates the weights
    clean, spans = S.parse_emphasis('a b (c d e:2)')
    assert S.emphasis_weights(tok, clean, spans, 3 * per) == ([1.0] * (2 * per) + [2.0] * per)


def test_a_boundary_inside_a_token_raises_naming_the_span():
    class Merging(WordTok):      # the ids of a prefix that ends inside a word are no prefix of the whole text's
        def __call__(self, text, add_special_tokens=True, **kw):
            return type('Enc', (), dict(input_ids=[sum(map(ord, w)) for w in text.split()] + ([1] if add_special_tokens else [])))()
    with pytest.raises(ValueError, match='ab'):
        S.emphasis_weights(Merging(), 'xab c', [(1, 3, 2.0)], 8)


def test_new_symbols_are_exported():
    from ezaudio_amd import MaskDiT, _lib
    from ezaudio_amd.api import EzAudio, EzAudio_ControlNet
    import inspect
    assert hasattr(MaskDiT, 'set_context_token_weights')
    assert 'context_token_weights' in inspect.signature(MaskDiT.forward).parameters
    for name in ('token_weights', 'uncond_token_weights', 'compose_token_weights'):
        assert name in inspect.signature(_RealSampler.prepare).parameters
    for name in ('emphasis', 'token_weights'):
        assert name in inspect.signature(S.inference).parameters
    for fn in ('generate_audio', 'editing_audio', 'audio_to_audio', 'generate_long_audio', 'generate_loop'):
        assert inspect.signature(getattr(EzAudio, fn)).parameters['emphasis'].default is False
    assert 'emphasis' not in inspect.signature(EzAudio.generate_scene).parameters
    assert 'emphasis' not in inspect.signature(EzAudio_ControlNet.generate_audio).parameters
    lib = _lib.load()
    for sym in ('ezdit_set_context_token_weights', 'ezdit_test_attention_keyweights', 'ezdit_test_cross_attention_keyweights'):
        assert getattr(lib, sym) is not None


# ---- inference(): what reaches the sampler (a recording sampler; fakes of tests/test_ragged_host.py, a word tokenizer that serves both call forms)
class _BatchTok(WordTok):
    def __call__(self, texts, max_length=None, padding=None, truncation=None, return_tensors=None, add_special_tokens=True):
        import torch
        if isinstance(texts, str):
            return WordTok.__call__(self, texts, add_special_tokens=add_special_tokens)
        rows = [(WordTok.__call__(self, t).input_ids)[:max_length] for t in texts]
        ids = torch.tensor([r + [0] * (max_length - len(r)) for r in rows])
        return type('B', (), dict(input_ids=ids, attention_mask=(ids > 0).long()))()


class _Recorder:
    seen = []

    def __init__(self, unet, scheduler):
        pass

    def prepare(self, text, text_mask, uncond, uncond_mask, init, step_noises, gs, gr, steps, eta, **kw):
        _Recorder.seen.append(dict(text=text.clone(), uncond=uncond.clone(), kw=kw))
        self.lat = init

    def run(self, use_graph=True):
        pass

    def finish(self):
        return self.lat


def _infer(prompts, neg=None, **kw):
    from tests.test_ragged_host import PARAMS, _Unet, _enc, _vae
    args = dict(audio_frames=8, guidance_scale=5, guidance_rescale=0.0, ddim_steps=3, eta=0, random_seed=11)
    args.update(kw)
    S.inference(_vae, _Unet(), None, None, _BatchTok(), _enc, PARAMS, None, prompts, neg, device='cpu', **args)
    return _Recorder.seen[-1]


def test_inference_passes_the_table_on_only_when_a_weight_is_not_one(monkeypatch):
    import torch
    monkeypatch.setattr(S, 'LatentSampler', _Recorder)
    marked = 'a (dog barking:2) in rain'
    verbatim = _infer([marked])                                   # emphasis=False: the prompt is encoded as it stands, markup and all
    assert 'token_weights' not in verbatim['kw']
    assert torch.equal(verbatim['text'], _infer([marked], emphasis=False)['text'])
    on = _infer([marked], emphasis=True)
    clean = _infer(['a dog barking in rain'])
    assert torch.equal(on['text'], clean['text']) and not torch.equal(on['text'], verbatim['text'])      # the encoder sees the clean text
    assert on['kw']['token_weights'].tolist() == [[1.0, 2.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0]] and 'uncond_token_weights' not in on['kw']
    assert 'token_weights' not in _infer(['a (dog:1) barking in rain'], emphasis=True)['kw']             # all weights 1: no table
    assert 'token_weights' not in _infer(['no markup'], emphasis=True)['kw']
    neg = _infer(['rain'], neg=['(loud:3) music'], emphasis=True)
    assert neg['kw']['uncond_token_weights'].tolist() == [[3.0] + [1.0] * 7] and bool((neg['kw']['token_weights'] == 1).all())
    direct = _infer(['a dog barking in rain'], token_weights=on['kw']['token_weights'])
    assert torch.equal(direct['kw']['token_weights'], on['kw']['token_weights']) and torch.equal(direct['text'], on['text'])
    comp = _infer(['a (dog:2)'], compose=[('(loud:0.5) rain', 0.7)], emphasis=True)
    assert comp['kw']['token_weights'].tolist() == [[1.0, 2.0] + [1.0] * 6]
    assert comp['kw']['compose_token_weights'].tolist() == [[[0.5] + [1.0] * 7]]
    with pytest.raises(ValueError, match='timeline'):
        _infer([['a', 'b']], emphasis=True, prompt_weights=[torch.ones(2, 8)])


@pytest.mark.parametrize('name', ['xs', 'xs64'])
def test_stored_weighted_goldens_lie_five_gates_from_the_unweighted_result(name):
    """tools/mint_emphasis_golden.py: a condition on the stored arrays, not a measurement -- both sets at the first timestep, at least 1e-1 rel-L2 from the unweighted oracle
    result stored beside them; the subclass that minted the fractional set reproduced the duplicated-context set within 20 times the oracle's permuted-rows floor."""
    from tests.util import load_golden, rel_l2
    g, meta = load_golden('forward_emphasis_' + name)
    t0 = meta['timesteps'][0]
    for kind in ('int', 'frac'):
        d = rel_l2(g[f'pred_{kind}_t{t0}'], g[f'plain_t{t0}'])
        print(name, kind, 'from the unweighted result: %.3e' % d)
        assert d >= 1e-1, (kind, d)
        assert abs(d - meta[f'{kind}_vs_plain']) < 1e-6
    w = g['w_int']
    assert bool((w == w.round()).all()) and float(w.max()) > 1 and g['w_frac'].shape == w.shape == g['ctx'].shape[:2]
    floor = meta['permuted_rows_floor'][meta['pattern']]
    assert 0 < floor < 1e-6 and all(v <= 20 * floor for v in meta['subclass_vs_duplicated'].values())


def test_stored_loop_goldens_are_far_from_the_unweighted_loop():
    from tests.util import load_golden, rel_l2
    g, meta = load_golden('sampler_emphasis_xs')
    base, _ = load_golden('sampler_smp_xs_e0')
    assert meta['base'] == 'smp_xs_e0' and meta['steps'] == 20
    assert rel_l2(g['latent_ddim'], base['latent']) >= 1e-1
    assert g['latent_dpmpp_2m'].shape == g['latent_ddim'].shape and bool((g['weights'] != 1).any())
