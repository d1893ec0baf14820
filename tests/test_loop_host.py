"""CPU tests of the host side of seamless loops (the canvas as a ring, blended inside the step, decoded with wrapped context): loop_windows,
check_canvas_loop, draw_noises(canvas_loop=), decode_circular and Autoencoder.decoder_context_frames against the numpy VAE oracle, EzAudio.generate_loop's
bookkeeping against a recording sampler and a stub VAE (the pattern of tests/test_canvas_host.py; the stand-ins are copied, not imported from a test module),
and the two new entry points of the C ABI."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ezaudio_amd.sampler import LatentSampler as _RealSampler
from ezaudio_amd.vae import Autoencoder
from tests.util import DIFF, record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {'text_encoder': {'max_length': 8}, 'model': {'out_chans': 4},
          'autoencoder': {'scale': 0.5, 'shift': -0.25, 'sr': 80, 'latent_sr': 10, 'dim': 4}}
SR, RATIO, DIM = 80, 8, 4
MINI_VAE = dict(channels=64, c_mults=[1, 2], strides=[2, 4], latent_dim=128, out_channels=1)   # the decoder of the GPU tests' mini autoencoder


# ---------------------------------------------------------------------------------------------------
# 1. the windows
# ---------------------------------------------------------------------------------------------------
def _qualifies(T, L, O, P):
    """P windows of L frames at i T // P on a ring of T: ascending, every frame covered, every cyclic neighbour overlap >= O (restated, not imported)."""
    offs = [i * T // P for i in range(P)]
    steps = [b - a for a, b in zip(offs, offs[1:] + [T])]
    return min(steps) >= 1 and all(L - s >= max(O, 0) for s in steps)


def test_loop_windows_exhaustive():
    from ezaudio_amd.sampler import check_canvas_loop, loop_overlaps, loop_windows
    assert loop_windows(300, 100, 25) == ([0, 75, 150, 225], 100)
    assert loop_windows(96, 96, 48) == ([0, 48], 96) and loop_windows(50, 96, 0) == ([0, 25], 50)       # a ring within one window: two, half a turn apart
    assert loop_windows(170, 96, 30) == ([0, 56, 113], 96)
    n = 0
    for window in (50, 96):
        for O in (0, 1, 24):
            for T in range(2, 401):
                L = min(window, T)
                if O >= L:                                                   # no P <= T shares that much: even steps of 1 share L - 1
                    assert not any(_qualifies(T, L, O, P) for P in range(2, T + 1))
                    with pytest.raises(ValueError):
                        loop_windows(T, window, O)
                    continue
                offs, win = loop_windows(T, window, O)
                P = len(offs)
                assert win == L and L <= T and P >= 2 and offs == [i * T // P for i in range(P)], (T, window, O)
                held = np.zeros(T, np.int64)
                for o in offs:
                    held[(o + np.arange(L)) % T] += 1
                assert held.min() >= 1, (T, window, O)                       # every frame is covered
                ov = loop_overlaps(offs, L, T)
                assert len(ov) == P and min(ov) >= O and ov[-1] == offs[-1] + L - T, (T, window, O, offs)
                assert _qualifies(T, L, O, P) and not any(_qualifies(T, L, O, q) for q in range(2, P)), (T, window, O, P)
                check_canvas_loop(offs, L, T, max(1, min(ov)))
                n += 1
    assert n > 2000
    for bad in ((1, 96, 0), (0, 96, 0), (300, 0, 0), (300, 96, -1), (300, 96, 96), (10, 96, 10)):
        with pytest.raises(ValueError):
            loop_windows(*bad)


def test_check_canvas_loop_refuses_each_broken_rule():
    from ezaudio_amd.sampler import check_canvas_loop
    for offs, L, T, ramp in (([0, 52, 104], 96, 170, 30), ([0, 52, 104], 96, 200, 1), ([0, 48], 96, 96, 48), ([0, 30, 60], 96, 100, 1), ([0], 96, 96, 1),
                             ([0, 149, 298], 150, 447, 1)):
        check_canvas_loop(offs, L, T, ramp)
    for what, (offs, L, T, ramp) in (('first offset', ([1, 52, 104], 96, 170, 30)), ('not ascending', ([0, 104, 104], 96, 170, 30)),
                                     ('descending', ([0, 104, 52], 96, 170, 30)), ('a gap between neighbours', ([0, 97, 104], 96, 170, 30)),
                                     ('last offset at T', ([0, 52, 104], 96, 104, 30)), ('last offset beyond T', ([0, 90, 180], 96, 170, 30)),
                                     ('a gap at the wrap', ([0, 52, 104], 96, 201, 30)), ('L > T', ([0, 48], 96, 95, 30)), ('ramp 0', ([0, 52, 104], 96, 170, 0)),
                                     ('no window', ([], 96, 96, 1))):
        with pytest.raises(ValueError):
            check_canvas_loop(offs, L, T, ramp)
            pytest.fail(what)


# ---------------------------------------------------------------------------------------------------
# 2. the draws
# ---------------------------------------------------------------------------------------------------
def test_draw_noises_with_canvas_loop_cuts_one_ring_draw_with_wrap():
    from ezaudio_amd.sampler import draw_noises
    K, offs, L, T = 5, [0, 4, 8], 6, 11
    init, step = draw_noises(4, L, K, 1, 12, 'cpu', n_prompts=3, canvas_offsets=offs, canvas_loop=T)
    assert init.shape == (3, 4, L) and step.shape == (K, 3, 4, L)
    g = torch.Generator().manual_seed(12)
    ring = torch.randn((1, 4, T), generator=g)
    ix = [[(o + r) % T for r in range(L)] for o in offs]
    for i in range(3):
        assert torch.equal(init[i:i + 1], ring[:, :, ix[i]])
    assert torch.equal(init[0, :, 4:], init[1, :, :2])                      # windows agree where they share ring frames ...
    assert torch.equal(init[2, :, 3:], init[0, :, :3])                      # ... through the wrap too: window 2 holds 8, 9, 10, 0, 1, 2
    for k in range(K):
        z = torch.randn((1, 4, T), generator=g)
        for i in range(3):
            assert torch.equal(step[k, i:i + 1], z[:, :, ix[i]]), (k, i)
        assert torch.equal(step[k, 2, :, 3:], step[k, 0, :, :3])
    i0, s0 = draw_noises(4, L, K, 0, 12, 'cpu', n_prompts=3, canvas_offsets=offs, canvas_loop=T)
    assert torch.equal(i0, init) and s0 is None                             # eta 0 draws nothing per step
    # the draw order is the plain single-prompt call's of T frames: the first tensor is its init noise
    plain_i, plain_s = draw_noises(4, T, K, 1, 12, 'cpu', n_prompts=1)
    assert torch.equal(plain_i, ring) and torch.equal(init[0:1], plain_i[:, :, :L]) and torch.equal(step[0, 0:1], plain_s[0][:, :, :L])
    # a table without wrap is the linear canvas' draw; without the keyword nothing changes
    lin = draw_noises(4, L, K, 1, 12, 'cpu', n_prompts=3, canvas_offsets=[0, 4, 9])
    same = draw_noises(4, L, K, 1, 12, 'cpu', n_prompts=3, canvas_offsets=[0, 4, 9], canvas_loop=15)
    assert torch.equal(lin[0], same[0]) and torch.equal(lin[1], same[1])
    assert inspect.signature(draw_noises).parameters['canvas_loop'].default is None
    for bad in (dict(canvas_offsets=None), dict(canvas_loop=5), dict(eta=[1, 1, 1]), dict(random_seed=[1, 2, 3])):
        kw = dict(codec_dim=4, audio_frames=L, ddim_steps=K, eta=1, random_seed=12, device='cpu', n_prompts=3, canvas_offsets=offs, canvas_loop=T)
        kw.update(bad)
        with pytest.raises(ValueError):
            draw_noises(**kw)


# ---------------------------------------------------------------------------------------------------
# 3. the circular decode: the receptive field from the layer list, against the numpy VAE oracle
# ---------------------------------------------------------------------------------------------------
class _OracleAE:
    """The numpy decoder oracle behind the autoencoder's call surface (no decoder_context_frames: an injected autoencoder)."""

    def __init__(self, dec):
        self.dec, self.calls = dec, 0

    def __call__(self, embedding=None):
        self.calls += 1
        return torch.from_numpy(self.dec(embedding.numpy()))


def test_decoder_context_frames_is_the_receptive_field_of_the_oracle_decoder(lib):
    """decode_circular with decoder_context_frames() wrapped frames against the middle third of the decode of the latent tiled three times (no kept sample of
    that third is within a tile of a zero halo), numpy oracle, fp32.  Gate 1e-6 rel-L2: both run the same fp32 operations on the same values, only the BLAS
    shapes differ (fp32 epsilon 6e-8); measured 0, bitwise.  With context - 1 one side misses one frame: the outermost samples must differ by more than 1e-5
    (a hundred epsilons of the 1.7 amplitude; measured 6.0e-5), so the number is exact, not merely sufficient.  Also the real decoder's layer list by hand."""
    from ezaudio_amd.sampler import decode_circular
    from ezaudio_amd.vae import OobleckDecoder
    from oracle import vae as V
    from oracle.weights import uniform_pm1
    mini = OobleckDecoder(device='cpu', **MINI_VAE)
    ctx = mini.context_frames()
    # by hand, backwards from the 8 samples of one latent frame: conv_out 3; units 39; up k 4 s 2 p 1; units 39; up k 8 s 4 p 2; conv_in 3
    lo, hi = 0 - 3 - 39, 7 + 3 + 39
    lo, hi = -((4 - 1 - 1 - lo) // 2), (hi + 1) // 2
    lo, hi = lo - 39, hi + 39
    lo, hi = -((8 - 1 - 2 - lo) // 4), (hi + 2) // 4
    assert ctx == max(3 - lo, hi + 3) == 19
    assert [l[0] for l in mini.layer_list()] == ['conv', 'up', 'conv', 'conv', 'conv', 'up', 'conv', 'conv', 'conv', 'conv']
    assert OobleckDecoder(device='cpu').context_frames() == 9 and OobleckDecoder(device='cpu', strides=(2, 2, 2, 2)).context_frames() > 19   # not a constant
    ae = Autoencoder.__new__(Autoencoder)
    ae.ae = type('AE', (), dict(decoder=mini))()
    assert ae.decoder_context_frames() == ctx
    dec = _OracleAE(V.DecoderOracle(MINI_VAE, V.make_vae_state_dict(MINI_VAE, 5)))
    T = 2 * ctx + 3
    z = torch.from_numpy(uniform_pm1('loop.decode', 128 * T, 3).reshape(1, 128, T).astype(np.float32))
    ref = dec(embedding=z.repeat(1, 1, 3))[..., T * 8:2 * T * 8].numpy().astype(np.float64)
    rel = lambda w: float(np.linalg.norm(w.numpy() - ref) / np.linalg.norm(ref))   # noqa: E731
    dec.calls = 0
    got = decode_circular(dec, z, ctx)
    assert dec.calls == 1 and got.shape == (1, 1, T * 8)
    record(f'decode_circular, numpy oracle, mini decoder, T {T}, context {ctx}: rel-L2 vs the middle third of the tiled decode {rel(got):.3e} '
           f'(bitwise: {np.array_equal(got.numpy(), ref.astype(np.float32))})')
    assert rel(got) <= 1e-6
    short = decode_circular(dec, z, ctx - 1)
    edge = max(np.abs(short.numpy()[0, 0, :8] - ref[0, 0, :8]).max(), np.abs(short.numpy()[0, 0, -8:] - ref[0, 0, -8:]).max())
    record(f'decode_circular with context {ctx - 1}: largest difference on the outermost latent frames {edge:.3e}')
    assert short.shape == got.shape and edge > 1e-5
    # context beyond the ring tiles it; more context changes nothing
    assert rel(decode_circular(dec, z, 2 * T + 5)) <= 1e-6
    # rolling the ring rolls the waveform
    assert rel(torch.roll(decode_circular(dec, torch.roll(z, 5, dims=2), ctx), -5 * 8, dims=2)) <= 1e-6
    with pytest.raises(ValueError, match='context'):
        decode_circular(dec, z)                                              # an injected autoencoder without the method needs an explicit value
    dec.decoder_context_frames = lambda: ctx
    assert torch.equal(decode_circular(dec, z), got)
    with pytest.raises(ValueError):
        decode_circular(dec, z, -1)


# ---------------------------------------------------------------------------------------------------
# 4. EzAudio.generate_loop against stand-ins
# ---------------------------------------------------------------------------------------------------
class _RecordingSampler:
    """Keeps what prepare() was given; its windows are their init noise plus a per-window constant, its ring the real assembly rule (lowest window wins)."""
    seen = []

    def __init__(self, unet, scheduler):
        pass

    def prepare(self, text, text_mask, uncond, uncond_mask, init, step_noises, gs, gr, steps, eta, gt=None, gt_mask=None,
                controlnet=None, condition=None, conditioning_scale=1.0, **kw):
        P, _, L = init.shape
        self.lat = init + text.mean(dim=(1, 2))[:, None, None]
        self.ring = kw.get('canvas_loop')
        _RecordingSampler.seen.append(dict(P=P, L=L, init=init.clone(), step_noises=step_noises, gt=gt, kw=dict(kw), gs=gs, gr=gr, eta=eta, steps=steps,
                                           text=text.clone()))

    def run(self, use_graph=True):
        pass

    def finish(self):
        return self.lat

    def canvas_latents(self):
        offs, T, _ = self.ring
        out = torch.empty(1, self.lat.shape[1], T)
        for p in reversed(range(len(offs))):
            out[0, :, [(offs[p] + r) % T for r in range(self.lat.shape[2])]] = self.lat[p]
        return out


class _Tok:
    def __call__(self, texts, max_length, padding, truncation, return_tensors):
        ids = torch.tensor([[len(t) + 1, (sum(map(ord, t)) % 50) + 1] + [0] * (max_length - 2) for t in texts])
        return type('B', (), dict(input_ids=ids, attention_mask=(ids > 0).long()))()


def _enc(input_ids, attention_mask):
    return type('O', (), dict(last_hidden_state=torch.sin(input_ids.float())[:, :, None].repeat(1, 1, 6)))()


class _Unet:
    def eval(self):
        return self


class _StubVAE(Autoencoder):
    """Every sample is the mean of its latent frame and both neighbours: a receptive field of one frame, zero halos like the real decoder."""

    def __init__(self):
        self.calls = []

    def decoder_context_frames(self):
        return 1

    def __call__(self, audio=None, embedding=None, lengths=None):
        self.calls.append(('decode', tuple(embedding.shape), None if lengths is None else list(lengths)))
        x = torch.nn.functional.pad(embedding[:, :1], (1, 1))
        return ((x[..., :-2] + x[..., 1:-1] + x[..., 2:]) / 3).repeat_interleave(RATIO, dim=2).clone()


def _ez():
    from ezaudio_amd import api
    from ezaudio_amd.scheduler import DDIMScheduler
    ez = api.EzAudio.__new__(api.EzAudio)
    ez.device = 'cpu'
    ez.autoencoder, ez.unet, ez.tokenizer, ez.text_encoder, ez.noise_scheduler, ez.params = _StubVAE(), _Unet(), _Tok(), _enc, DDIMScheduler(**DIFF), PARAMS
    return ez


@pytest.fixture()
def seen(monkeypatch):
    from ezaudio_amd import sampler as S
    monkeypatch.setattr(S, 'LatentSampler', _RecordingSampler)
    _RecordingSampler.seen.clear()
    return _RecordingSampler.seen


def test_generate_loop_is_one_sampler_call_and_one_circular_decode(seen):
    from ezaudio_amd.sampler import draw_noises, loop_windows
    ez = _ez()
    # 30 s at 10 latent frames per second in windows of 10 s that share 2.5 s: a ring of 300 frames in windows of 100 sharing >= 25
    offs, L = loop_windows(300, 100, 25)
    assert offs == [0, 75, 150, 225] and L == 100
    sr, wav = ez.generate_loop('rain on a roof', 30, ddim_steps=20, random_seed=7)
    assert sr == SR and isinstance(wav, np.ndarray) and wav.shape == (300 * RATIO,)
    assert len(seen) == 1 and ez.autoencoder.calls == [('decode', (1, DIM, 302), None)]          # one decode, one wrapped frame on either side
    b = seen[0]
    assert b['P'] == 4 and b['L'] == 100 and b['steps'] == 20 and b['gt'] is None and (b['gs'], b['gr'], b['eta']) == (5, 0.75, 1)
    assert set(b['kw']) == {'canvas_loop'} and b['kw']['canvas_loop'] == (offs, 300, 25)         # the ramp: the smallest cyclic overlap
    init, step = draw_noises(DIM, 100, 20, 1, 7, 'cpu', n_prompts=4, canvas_offsets=offs, canvas_loop=300)
    assert torch.equal(b['init'], init) and torch.equal(b['step_noises'], step)
    assert torch.equal(init[3, :, 75:], init[0, :, :25])                                         # the last window runs into the first
    # the waveform is the circular decode of the ring in VAE space: its first sample has seen the last frame
    ring = torch.empty(1, DIM, 300)
    lat = init + b['text'].mean(dim=(1, 2))[:, None, None]
    for p in reversed(range(4)):
        ring[0, :, [(offs[p] + r) % 300 for r in range(100)]] = lat[p]
    z = (ring / 0.5 + 0.25)[0, 0]
    want = ((torch.roll(z, 1) + z + torch.roll(z, -1)) / 3).repeat_interleave(RATIO).numpy()
    assert np.array_equal(wav, want)
    # one prompt per window, the 2M solver, more context
    seen.clear()
    ez.generate_loop(['rain', 'thunder', 'rain', 'birds'], 30, ddim_steps=20, random_seed=7, eta=0, solver='dpmpp_2m', decode_context=4)
    assert len(seen) == 1 and seen[0]['kw'] == dict(canvas_loop=(offs, 300, 25), solver='dpmpp_2m') and seen[0]['step_noises'] is None
    assert ez.autoencoder.calls[-1] == ('decode', (1, DIM, 308), None)
    assert not torch.equal(seen[0]['text'][0], seen[0]['text'][1]) and torch.equal(seen[0]['text'][0], seen[0]['text'][2])
    # a loop no longer than the window: two windows of its own length, half a turn apart; any length of at least 2 frames
    for length, want_kw in ((7, ([0, 35], 70, 35)), (10, ([0, 50], 100, 50)), (0.2, ([0, 1], 2, 1)), (15, ([0, 75], 150, 25))):
        seen.clear()
        sr, wav = ez.generate_loop('rain', length, ddim_steps=20, random_seed=1)
        assert seen[0]['kw']['canvas_loop'] == want_kw and seen[0]['P'] == 2 and wav.shape == (want_kw[1] * RATIO,), length


def test_generate_loop_refusals(seen):
    ez = _ez()
    with pytest.raises(ValueError, match='4 windows'):
        ez.generate_loop(['rain', 'thunder'], 30, ddim_steps=20)
    with pytest.raises(ValueError, match='2 windows'):
        ez.generate_loop(['rain'], 10, ddim_steps=20)
    for kw in (dict(guidance_scale=[5] * 4), dict(eta=[1] * 4), dict(random_seed=[1] * 4), dict(guidance_rescale=[0.5] * 4), dict(ddim_steps=[20] * 4),
               dict(solver='dpmpp_2m'), dict(solver='unipc'), dict(overlap=10), dict(overlap=-1)):
        with pytest.raises(ValueError):
            ez.generate_loop('rain', 30, **{**dict(ddim_steps=20), **kw})
    for length in ([30, 30], 0.1, 0):
        with pytest.raises(ValueError):
            ez.generate_loop('rain', length)
    assert not seen and not ez.autoencoder.calls


def test_inference_loop_keywords_and_refusals(seen):
    from ezaudio_amd.sampler import inference
    names = list(inspect.signature(inference).parameters)
    assert names[-5:] == ['canvas_loop', 'decode_context', 'canvas_offsets', 'canvas_ramp', 'solver']     # the line's keywords stay where they were
    sig = inspect.signature(_RealSampler.prepare).parameters
    assert sig['canvas_loop'].default is None and list(sig)[-3:] == ['canvas', 'canvas_loop', 'solver']
    ez = _ez()
    args = (ez.autoencoder, ez.unet, None, None, ez.tokenizer, ez.text_encoder, PARAMS, ez.noise_scheduler)
    rest = (None, 6, 3, 0.0, 20, 0, 1, 'cpu')
    out = inference(*args, 'rain', *rest, canvas_offsets=[0, 4, 8], canvas_loop=11, canvas_ramp=1)
    assert out.shape == (1, 1, 11 * RATIO) and seen[0]['kw'] == dict(canvas_loop=([0, 4, 8], 11, 1)) and seen[0]['P'] == 3
    inference(*args, ['rain', 'wind', 'sea'], *rest, canvas_offsets=[0, 4, 8], canvas_loop=12)
    assert seen[1]['kw']['canvas_loop'] == ([0, 4, 8], 12, 2)                # the smallest cyclic overlap: 6 - 4
    n = len(seen)
    lat = torch.zeros(1, 4, 6)
    for text, kw in ((['rain', 'wind'], dict(canvas_offsets=[0, 4, 8], canvas_loop=11)), ('rain', dict(canvas_loop=11)),
                     ('rain', dict(canvas_offsets=[0, 4, 8], canvas_loop=15)), ('rain', dict(canvas_offsets=[0, 4, 8], canvas_loop=8)),
                     ('rain', dict(canvas_offsets=[0, 4], canvas_loop=5)), ('rain', dict(canvas_offsets=[0, 4, 8], canvas_loop=11, canvas_ramp=0)),
                     ('rain', dict(canvas_offsets=[0, 4, 9], decode_context=3)), ('rain', dict(decode_context=3)),
                     ('rain', dict(canvas_offsets=[0, 4], canvas_loop=8, init_latents=lat, strength=0.5))):
        with pytest.raises(ValueError):
            inference(*args, text, *rest, **kw)
    with pytest.raises(ValueError):
        inference(*args[:2], lat, lat.bool(), *args[4:], 'rain', *rest, canvas_offsets=[0, 4], canvas_loop=8)
    assert len(seen) == n


# ---------------------------------------------------------------------------------------------------
# 5. ABI
# ---------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_binding_binds_the_loop_entry_points(lib):
    from ezaudio_amd import _lib
    from oracle.weights import model_config
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ezdit.h')).read(), flags=re.S)
    for name, nargs in (('ezdit_canvas_blend_loop', 8), ('ezdit_sampler_set_canvas_loop', 6)):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m and len(m.group(1).split(',')) == nargs, name
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib, name).argtypes == args                                                          # exported and bound
    assert '#define EZDIT_ABI_VERSION 4' in hdr and lib.ezdit_abi_version() == 4 and _lib.ABI_VERSION == 4    # additive: the version stays
    cfg = model_config('xs')
    c = _lib.EzditConfig(cfg['embed_dim'], cfg['num_heads'], cfg['depth'], cfg['in_chans'], cfg['out_chans'], cfg['context_dim'],
                         cfg['ada_sola_rank'], float(cfg['ada_sola_alpha']), float(cfg['mlp_ratio']), 2048)
    h = C.c_void_p()
    assert lib.ezdit_create(C.byref(c), C.byref(h)) == 0
    try:
        off = (C.c_int32 * 2)(0, 50)
        assert lib.ezdit_sampler_set_canvas_loop(h, off, 2, 120, 1, None) == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_set_canvas_loop(h, None, 0, 0, 1, None) == -3
        assert lib.ezdit_sampler_set_canvas_loop(None, off, 2, 120, 1, None) == -1
        assert lib.ezdit_workspace_bytes(h, 6, 96, 20, 20) > 0
    finally:
        lib.ezdit_destroy(h)
    # refused before anything is launched: null pointers, ramp 0, L > T, a T that no table of P windows of L frames covers
    assert lib.ezdit_canvas_blend_loop(None, None, 3, 128, 96, 170, 1, None) == -1
    assert lib.ezdit_canvas_blend_loop(C.c_void_p(256), None, 3, 128, 96, 170, 1, None) == -1
    assert lib.ezdit_canvas_blend_loop(None, C.c_void_p(256), 3, 128, 96, 170, 1, None) == -1
    for P, Cc, L, T, ramp in ((3, 128, 96, 170, 0), (3, 128, 96, 95, 1), (3, 128, 96, 289, 1), (0, 128, 96, 96, 1), (3, 0, 96, 170, 1), (3, 128, 0, 170, 1)):
        assert lib.ezdit_canvas_blend_loop(C.c_void_p(256), C.c_void_p(256), P, Cc, L, T, ramp, None) == -1, (P, Cc, L, T, ramp)
        assert lib.ezdit_last_error()
