"""The host side of the prompt timeline (no GPU): scene_weights, the 128-aligned context builder, the weights of a call, and the refusals of inference()."""
import pytest
import torch

from ezaudio_amd import sampler as SM


def test_scene_weights_columns_sum_to_one_and_ramp_over_the_crossfade():
    prompts, W = SM.scene_weights([('rain', 0, 5), ('a door slams', 5, 10)], 250, 25, 1.0)
    assert prompts == ['rain', 'a door slams'] and tuple(W.shape) == (2, 250) and W.dtype == torch.float32
    assert torch.allclose(W.sum(0), torch.ones(250), atol=1e-6)
    assert bool((W[0, :112] == 1).all()) and bool((W[1, :112] == 0).all())          # before 4.5 s: the first prompt alone
    assert bool((W[1, 138:] == 1).all()) and bool((W[0, 138:] == 0).all())          # behind 5.5 s: the second alone
    ramp = W[1, 113:137]
    assert bool((ramp[1:] > ramp[:-1]).all()) and abs(float(W[0, 124]) - 0.52) < 1e-6 and abs(float(W[1, 125]) - 0.52) < 1e-6      # linear, centred on 5 s
    assert float(W[0, 0]) == 1.0 and float(W[1, 249]) == 1.0                        # the clip's own edges are not ramped


def test_scene_weights_overlap_weight_and_hard_switch():
    _, W = SM.scene_weights([('a', 0, 10), ('b', 2, 4, 3.0)], 100, 10, 0.0)
    assert torch.allclose(W.sum(0), torch.ones(100), atol=1e-6)
    assert bool((W[1, 20:40] == 0.75).all()) and bool((W[0, 20:40] == 0.25).all())
    assert bool((W[1, :20] == 0).all()) and bool((W[1, 40:] == 0).all()) and bool((W[0, :20] == 1).all())


def test_scene_weights_refusals():
    with pytest.raises(ValueError, match='covers frame'):
        SM.scene_weights([('a', 0, 4), ('b', 6, 10)], 100, 10, 0.5)
    with pytest.raises(ValueError, match='outside the clip'):
        SM.scene_weights([('a', 0, 12)], 100, 10, 0.5)
    with pytest.raises(ValueError, match='outside the clip'):
        SM.scene_weights([('a', 3, 3)], 100, 10, 0.5)
    with pytest.raises(ValueError, match='between 1 and 16'):
        SM.scene_weights([('a', 0, 10)] * 17, 100, 10, 0.5)
    with pytest.raises(ValueError, match='between 1 and 16'):
        SM.scene_weights([], 100, 10, 0.5)
    with pytest.raises(ValueError, match='weight'):
        SM.scene_weights([('a', 0, 10, 0.0)], 100, 10, 0.5)


def test_timeline_context_puts_each_prompt_at_the_front_of_its_128_rows():
    g = torch.Generator().manual_seed(3)
    text = torch.randn(2, 3, 100, 8, generator=g)
    mask = torch.rand(2, 3, 100, generator=g) > 0.3
    ctx, msk = SM.timeline_context(text, mask)
    assert tuple(ctx.shape) == (2, 384, 8) and tuple(msk.shape) == (2, 384) and msk.dtype == torch.bool
    for s in range(3):
        assert torch.equal(ctx[:, 128 * s:128 * s + 100], text[:, s]) and torch.equal(msk[:, 128 * s:128 * s + 100], mask[:, s])
        assert bool((ctx[:, 128 * s + 100:128 * s + 128] == 0).all()) and not bool(msk[:, 128 * s + 100:128 * s + 128].any())
    with pytest.raises(ValueError):
        SM.timeline_context(torch.zeros(1, 129, 8), torch.zeros(1, 129))
    with pytest.raises(ValueError):
        SM.timeline_context(torch.zeros(17, 4, 8), torch.zeros(17, 4))


def test_the_weights_of_a_call_pad_missing_prompts_and_frames_with_zero():
    w0 = torch.rand(3, 80) + 0.1
    entries, W = SM._timeline_entries([['a', 'b', 'c'], 'd', ['e', 'f']], [w0, None, torch.ones(2, 33)], [80, 96, 33])
    assert entries == [['a', 'b', 'c'], ['d'], ['e', 'f']] and tuple(W.shape) == (3, 3, 96)
    assert torch.equal(W[0, :, :80], w0) and bool((W[0, :, 80:] == 0).all())
    assert bool((W[1, 0] == 1).all()) and bool((W[1, 1:] == 0).all())
    assert bool((W[2, :2, :33] == 1).all()) and bool((W[2, 2] == 0).all()) and bool((W[2, :, 33:] == 0).all())
    with pytest.raises(ValueError, match='no prompt_weights'):
        SM._timeline_entries([['a', 'b']], None, [10])
    with pytest.raises(ValueError, match='shape'):
        SM._timeline_entries([['a', 'b']], [torch.ones(2, 11)], [10])
    with pytest.raises(ValueError, match='entries of prompt_weights'):
        SM._timeline_entries(['a', 'b'], [None], [10, 10])


def _inference(**kw):
    args = dict(autoencoder=None, unet=None, gt=None, gt_mask=None, tokenizer=None, text_encoder=None, params={}, noise_scheduler=None,
                text_raw=[['a', 'b']], prompt_weights=[torch.ones(2, 10)], audio_frames=10, eta=0)
    args.update(kw)
    return SM.inference(**args)


def test_inference_refuses_a_timeline_with_a_canvas_a_controlnet_or_a_sharded_call(monkeypatch):
    with pytest.raises(ValueError, match='canvas or a ControlNet'):
        _inference(canvas_offsets=[0])
    with pytest.raises(ValueError, match='canvas or a ControlNet'):
        _inference(controlnet=object(), condition=torch.zeros(1, 1, 20))
    import torch.distributed as dist
    monkeypatch.setattr(dist, 'is_available', lambda: True)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda: 2)
    with pytest.raises(ValueError, match='not sharded'):
        _inference(text_raw=[['a', 'b'], 'c'], prompt_weights=[torch.ones(2, 10), None])
    monkeypatch.undo()
    with pytest.raises(NotImplementedError):      # a well-formed timeline call gets as far as the (missing) tokenizer
        _inference()


def _api():
    from ezaudio_amd import api
    ez = api.EzAudio.__new__(api.EzAudio)
    ez.params = {'autoencoder': {'latent_sr': 10, 'sr': 100}}
    ez.autoencoder = ez.unet = ez.tokenizer = ez.text_encoder = ez.noise_scheduler = None
    ez.device = 'cpu'
    return api, ez


def test_generate_scene_with_one_entry_is_generate_audio_of_that_text(monkeypatch):
    api, ez = _api()
    seen = []
    monkeypatch.setattr(ez, 'generate_audio', lambda *a, **kw: seen.append((a, kw)) or (100, 'wave'), raising=False)
    assert ez.generate_scene([('rain', 0, 4)], 4, random_seed=7, eta=0, solver='dpmpp_2m') == (100, 'wave')
    assert seen == [(('rain', 4, 5, 0.75, 100, 0, 7, False), dict(attention_window=None, solver='dpmpp_2m'))]


def test_generate_scene_hands_inference_one_entry_of_prompts_with_their_weights(monkeypatch):
    api, ez = _api()
    got = {}

    def fake(*a, **kw):
        got['a'], got['kw'] = a, kw
        return torch.zeros(1, 1, 400)
    monkeypatch.setattr(api, 'inference', fake)
    sr, wav = ez.generate_scene([('rain', 0, 2), ('a door slams', 2, 4)], 4, crossfade=0.5, random_seed=3)
    assert sr == 100 and wav.shape == (400,)
    assert got['a'][8] == [['rain', 'a door slams']] and got['a'][10] == 40 and got['kw']['attention_window'] is None
    (W,) = got['kw']['prompt_weights']
    assert tuple(W.shape) == (2, 40) and torch.allclose(W.sum(0), torch.ones(40), atol=1e-6) and float(W[0, 0]) == 1 and float(W[1, 39]) == 1
    with pytest.raises(ValueError, match='one clip'):
        ez.generate_scene([('rain', 0, 2), ('a door slams', 2, 4)], 4, eta=[0, 1])
