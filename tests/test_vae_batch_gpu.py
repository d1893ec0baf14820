"""The batched Oobleck VAE on the GPU: B samples, ragged or of one length, stacked along the token axis with zero gaps and run as ONE layer sequence
(ezaudio_amd/vae.py, the *_seg kernels of csrc/vae.hip).  Every sample must come out as the call with it alone gives it -- bit for bit, since each output row of
the GEMM depends on its own operand rows only -- within the oracle gates of tests/test_vae.py, and exactly zero beyond its own length; the padding is NaN, so
anything that reads it shows."""
import functools

import numpy as np
import pytest

from oracle import vae as V
from oracle.weights import uniform_pm1
from tests.util import record, rel_l2

pytestmark = pytest.mark.gpu

VAE_REL, VAE_MAX = 2e-2, 0.06            # the gates of tests/test_vae.py
MINI_VAE = dict(channels=64, c_mults=[1, 2], strides=[2, 4], latent_dim=128, out_channels=1)   # the mini VAE of tests/test_vae.py
CONFIGS = {'default': (dict(V.VAE_DEFAULT), 6), 'mini': (MINI_VAE, 5)}
DEC_LENS = [16, 9, 1, 13]                # one sample shorter than every halo of the residual units, one a single frame
ENC_T = [480 * 9 + 317, 480, 480 * 5 + 479, 480 * 3 + 1]   # every strided conv floors; a clip of minimum length; one a sample short of the next frame


@functools.lru_cache(maxsize=None)
def _state(name, encoder=False):
    cfg, seed = CONFIGS[name]
    return V.make_vae_state_dict(cfg, seed, encoder=encoder)


def _decoder(name):
    from ezaudio_amd.vae import OobleckDecoder
    cfg = CONFIGS[name][0]
    dec = OobleckDecoder(out_channels=1, channels=cfg['channels'], latent_dim=cfg['latent_dim'], c_mults=cfg['c_mults'], strides=cfg['strides'],
                         use_snake=True, final_tanh=False, device='cuda')
    return dec.load_state_dict(_state(name))


def _encoder(name):
    from ezaudio_amd.vae import OobleckEncoder
    cfg = CONFIGS[name][0]
    enc = OobleckEncoder(in_channels=1, channels=cfg['channels'], latent_dim=2 * cfg['latent_dim'], c_mults=cfg['c_mults'], strides=cfg['strides'],
                         use_snake=True, device='cuda')
    return enc.load_state_dict(_state(name, True))


@functools.lru_cache(maxsize=None)
def _latents(name, B, width):
    lat = CONFIGS[name][0]['latent_dim']
    z = (1.2 * uniform_pm1(f'vaeb_z_{name}', B * lat * width, 3)).reshape(B, lat, width).astype(np.float32)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _decoder_reference(name, b):
    """DecoderOracle on sample b of the ragged case alone (computed once per session)."""
    ref = V.DecoderOracle(CONFIGS[name][0], _state(name))(_latents(name, 4, 16)[b:b + 1, :, :DEC_LENS[b]])
    ref.setflags(write=False)
    return ref


def _padded(z, lens):
    """the samples at their own lengths, NaN behind"""
    out = np.full_like(z, np.nan)
    for b, n in enumerate(lens):
        out[b, :, :n] = z[b, :, :n]
    return out


@pytest.mark.parametrize('name', ['default', 'mini'])
def test_ragged_decode_is_each_sample_alone(name):
    import torch
    cfg = CONFIGS[name][0]
    ratio = int(np.prod(cfg['strides']))
    z = _latents(name, 4, 16)
    dec = _decoder(name)
    assert dec.latent_gap() == {'default': 3, 'mini': 7}[name]          # derived from the strides: 27 rows after the first up-sampling
    zp = torch.from_numpy(_padded(z, DEC_LENS)).cuda()
    out = dec(zp, lengths=DEC_LENS)
    assert tuple(out.shape) == (4, 1, 16 * ratio) and torch.isfinite(out).all()
    single = _decoder(name)
    for b, n in enumerate(DEC_LENS):
        ref = _decoder_reference(name, b)
        got = out[b:b + 1, :, :n * ratio].cpu().numpy()
        r = rel_l2(got, ref)
        m = np.abs(got - ref).max() / np.abs(ref).max()
        alone = single(torch.from_numpy(z[b:b + 1, :, :n].copy()).cuda())
        same = torch.equal(out[b:b + 1, :, :n * ratio], alone)
        record(f'ragged decode {name} sample {b} ({n} frames): rel_l2 {r:.3e} max/max {m:.3e} bit-identical to the single decode: {same}')
        assert r < VAE_REL and m < VAE_MAX
        assert same
        assert not out[b, :, n * ratio:].any()


def test_decode_writes_its_gap_rows_on_cached_buffers():
    """[16, 9] and then [9, 16] on the same object: the same total rows with the interiors swapped, so the cached buffers are not re-zeroed and the second call's
    gaps lie where the first call's interiors were."""
    import torch
    z = _latents('default', 4, 16)[:2]
    dec = _decoder('default')
    dec(torch.from_numpy(_padded(z, [16, 9])).cuda(), lengths=[16, 9])
    second = dec(torch.from_numpy(_padded(z, [9, 16])).cuda(), lengths=[9, 16])
    fresh = _decoder('default')(torch.from_numpy(_padded(z, [9, 16])).cuda(), lengths=[9, 16])
    assert torch.isfinite(second).all() and torch.equal(second, fresh)


def _count_gemms(net):
    calls = []
    real = net._gemm

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    net._gemm = counting
    return calls


def test_equal_length_batch_is_one_layer_sequence_and_the_single_decodes():
    import torch
    z = torch.from_numpy(_latents('default', 4, 16)[:3, :, :11].copy()).cuda()
    dec = _decoder('default')
    calls = _count_gemms(dec)
    one = [dec(z[b:b + 1]).clone() for b in range(3)]
    per_sample = len(calls) // 3
    del calls[:]
    out = dec(z)
    record(f'equal-length decode: {len(calls)} GEMM launches for 3 samples, {per_sample} for one')
    assert len(calls) == per_sample                                      # the count of ONE sample, not three
    for b in range(3):
        assert torch.equal(out[b:b + 1], one[b]), b
    # a batch above the GEMM's addressing limit is split into groups that stay below it (here: the limit lowered until two samples no longer fit one run)
    gap, width = dec.latent_gap(), 480 * 128
    dec.max_elems = (2 * (11 + gap) + 11 + 54) * width - 1
    del calls[:]
    grouped = dec(z)
    assert len(calls) == 2 * per_sample and torch.equal(grouped, out)


def test_ragged_encode_and_bottleneck_are_each_sample_alone():
    import torch
    from ezaudio_amd.vae import VAEBottleneck
    cfg = CONFIGS['default'][0]
    sd = _state('default', True)
    B, Tmax = len(ENC_T), max(ENC_T)
    wav = np.full((B, 1, Tmax), np.nan, np.float32)
    clips = [(0.5 * uniform_pm1(f'vaeb_wav{b}', T, 3)).astype(np.float32) for b, T in enumerate(ENC_T)]
    for b, c in enumerate(clips):
        wav[b, 0, :len(c)] = c
    enc = _encoder('default')
    assert enc.latent_lengths(ENC_T) == [T // 480 for T in ENC_T] == [9, 1, 5, 3]
    assert enc.sample_stride(Tmax) % 480 == 0 and enc.sample_stride(Tmax) - Tmax >= 27 * 48
    lat = enc(torch.from_numpy(wav).cuda(), lengths=ENC_T)
    assert tuple(lat.shape) == (B, 256, 9) and torch.isfinite(lat).all()
    single = _encoder('default')
    oracle = V.EncoderOracle(cfg, sd)
    refs = []
    for b, c in enumerate(clips):
        n = ENC_T[b] // 480
        ref = oracle(c.reshape(1, 1, -1))
        refs.append(ref)
        got = lat[b:b + 1, :, :n].cpu().numpy()
        assert ref.shape == got.shape
        r = rel_l2(got, ref)
        m = np.abs(got - ref).max() / np.abs(ref).max()
        alone = single(torch.from_numpy(c.reshape(1, 1, -1)).cuda())
        same = torch.equal(lat[b:b + 1, :, :n], alone)
        record(f'ragged encode sample {b} ({ENC_T[b]} samples): rel_l2 {r:.3e} max/max {m:.3e} bit-identical to the single encode: {same}')
        assert r < VAE_REL and m < VAE_MAX
        assert same
        assert not lat[b, :, n:].any()
    # the bottleneck on the oracle's means and scales, NaN behind each sample's frames, explicit noise
    L = [r.shape[2] for r in refs]
    x = np.full((B, 256, 9), np.nan, np.float32)
    noise = np.full((B, 128, 9), np.nan, np.float32)
    for b, r in enumerate(refs):
        x[b, :, :L[b]] = r[0]
        noise[b, :, :L[b]] = uniform_pm1(f'vaeb_noise{b}', 128 * L[b], 4).reshape(128, L[b])
    z = VAEBottleneck('cuda').encode(torch.from_numpy(x).cuda(), noise=torch.from_numpy(noise).cuda(), lengths=L).cpu().numpy()
    assert np.isfinite(z).all()
    for b, r in enumerate(refs):
        np.testing.assert_allclose(z[b:b + 1, :, :L[b]], V.vae_sample(r[:, :128], r[:, 128:], noise[b:b + 1, :, :L[b]]), rtol=1e-5, atol=1e-5)
        assert not z[b, :, L[b]:].any()
    # without noise: one draw per sample from the global generator, in order -- the draws of the single calls
    torch.manual_seed(5)
    drawn = VAEBottleneck('cuda').encode(torch.from_numpy(x).cuda(), lengths=L)
    torch.manual_seed(5)
    for b in range(B):
        alone = VAEBottleneck('cuda').encode(torch.from_numpy(x[b:b + 1, :, :L[b]].copy()).cuda())
        torch.testing.assert_close(drawn[b:b + 1, :, :L[b]], alone, rtol=1e-5, atol=1e-5)


def test_refusals():
    import torch
    from ezaudio_amd.vae import VAEBottleneck
    dec, enc = _decoder('mini'), _encoder('mini')
    z = torch.zeros(2, 128, 16, device='cuda')
    for bad in ([16], [16, 9, 4], [16, 0], [17, 9], [-1, 9]):
        with pytest.raises(ValueError):
            dec(z, lengths=bad)
    with pytest.raises(ValueError):
        dec(z[:1], lengths=[17])
    wav = torch.zeros(2, 1, 100, device='cuda')
    for bad in ([100], [100, 50, 50], [100, 0], [101, 50], [100, 7]):      # 7: shorter than the stride product 8
        with pytest.raises(ValueError):
            enc(wav, lengths=bad)
    with pytest.raises(ValueError):
        enc(wav[:1], lengths=[7])
    x = torch.zeros(2, 256, 12, device='cuda')
    for bad in ([12], [12, 0], [13, 2]):
        with pytest.raises(ValueError):
            VAEBottleneck('cuda').encode(x, lengths=bad)
    lib = dec.lib
    P = 4096                                                                 # never dereferenced: refused before any launch
    assert lib.ezvae_snake_bf16_seg(P, 64, None, None, P, 64, 0, 64, P, 2, 1, 1, 8, 8, None) == -1 and lib.ezdit_last_error()
    assert lib.ezvae_snake_bf16_seg(P, 64, None, None, P, 64, 16, 64, None, 2, 1, 1, 8, 8, None) == -1
    assert lib.ezvae_snake_bf16_seg(P, 64, None, None, P, 64, 16, 64, P, 2, 1, 0, 8, 8, None) == -1
    assert lib.ezvae_conv_out1_seg(P, 64, P, P, 16, 60, P, 2, 1, 1, 8, None) == -1
    assert lib.ezvae_conv_in1_seg(P, P, P, P, 16, 64, P, 0, 8, 8, None) == -1
    assert lib.ezvae_sample_seg(P, None, P, 2 ** 16, 2 ** 15, P, 2, 1, 1, 8, None) == -1
