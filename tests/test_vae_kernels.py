"""Kernel-level tests of the Oobleck VAE ops on the GPU: each public ezvae_* entry point, called directly through the C ABI, against a float64 reference of the same
operands (tests/vae_emul.py: cases, bounds and the reasons for them).  Every operand lies between NaN guards, every output in a sentinel-filled buffer, and a case passes
when (a) every owned element is within its bound, (b) the sentinel is intact everywhere else -- rows >= M, columns >= N up to ldo, halo and guard rows -- and (c) the
result is finite, i.e. nothing beyond the documented halo was read.  tests/test_vae.py shows on the CPU that these gates catch every addressing mistake of its list.
All references are computed on the CPU; the GPU only runs the op under test."""
import numpy as np
import pytest
import torch

from tests import vae_emul as E
from tests.util import record

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return DEV


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bf16(a):
    """float32 array of bf16 values (and NaN guards) -> bf16 on the device, exactly"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    b = t.to(torch.bfloat16)
    assert torch.equal(torch.nan_to_num(b.float()), torch.nan_to_num(t))
    return b.to(DEV)


def _run_gemm(lib, c, tile):
    a, w = _bf16(c.a), _bf16(E._guarded(c.w, 64))
    bias = None if c.bias is None else _f32(c.bias)
    r = None if c.r is None else _f32(c.r)
    out = _f32(c.out_alloc())
    rc = lib.ezvae_gemm(a.data_ptr() + c.a0 * 2, c.lda, w.data_ptr() + 64 * 2, c.K, c.N, None if bias is None else bias.data_ptr(),
                        None if r is None else r.data_ptr() + c.r0 * 4, c.ldr, out.data_ptr() + E.GUARD * c.ldo * 4, c.ldo, c.M, c.N, c.K, c.cpb, c.tap_bytes,
                        tile, None)
    assert rc == 0, (c.name, tile, lib.ezdit_last_error())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('tile', [6, 25])
@pytest.mark.parametrize('family', list(E.GEMM_FAMILIES))
def test_vae_gemm_family_against_fp64(lib, dev, family, tile):
    """Tile 6 (the VAE's) on every case of the family, tile 25 (the other 128 x 64 lockstep id, ring of 4) on one: per element
    |got - ref| <= (K + 3) 2^-24 (sum |a w| + |bias| + |resid|), rel-L2 < 1e-5, sentinel intact, finite."""
    specs = E.GEMM_FAMILIES[family] if tile == 6 else [E.GEMM_TILE25[family]]
    worst, worst_rel, failed = 0.0, 0.0, []
    for spec in specs:
        c = E.build(spec)
        ex, rl = c.measure(_run_gemm(lib, c, tile))
        print(f'{c.name} tile {tile}: excess {ex:.3e} rel_l2 {rl:.3e}')
        worst, worst_rel = max(worst, ex), max(worst_rel, rl)
        if not ex <= 1.0:
            failed.append((c.name, ex, rl))
    record(f'vae gemm {family} tile {tile}: {len(specs)} cases, worst error / bound {worst:.3e}, worst rel_l2 {worst_rel:.3e}')
    assert not failed, failed


def _run_snake(lib, c):
    x = _f32(c.x_alloc)
    al = None if c.alpha is None else _f32(c.alpha)
    ib = None if c.inv_beta is None else _f32(c.inv_beta)
    out = torch.from_numpy(c.out_alloc().view(np.int16)).to(DEV)
    rc = lib.ezvae_snake_bf16(x.data_ptr() + c.x0 * 4, c.ldx, None if al is None else al.data_ptr(), None if ib is None else ib.data_ptr(),
                              out.data_ptr() + c.out0 * 2, c.ldo, c.L, c.C, None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize('params', [False, True])
def test_vae_snake_bf16_against_fp64(lib, dev, params):
    """alpha NULL: the cast, bitwise round-to-nearest-even on ties, binade carries, signed zeros, the largest and the smallest magnitudes.  With parameters:
    within one bf16 ulp (+ the fp32 product's share) of float64 x + inv_beta sin(alpha x)^2 with |alpha x| up to 300, at most 0.5 % of the elements not bit-equal."""
    worst, worst_share, failed = 0.0, 0.0, []
    for C, L in E.SNAKE_SHAPES:
        c = E.SnakeCase(C, L, params)
        ex, share = c.measure(_run_snake(lib, c))
        print(f'snake C{C} L{L} params {params}: excess {ex:.3e} not bit-equal {share:.3e}')
        worst, worst_share = max(worst, ex), max(worst_share, share)
        if not ex <= 1.0:
            failed.append((C, L, ex, share))
    record(f'vae snake params {params}: worst error / bound {worst:.3e}, worst share not bit-equal {worst_share:.3e} (cap {E.SNAKE_SHARE_CAP:.1e})')
    assert not failed, failed


def test_vae_conv_out1_against_fp64(lib, dev):
    """C -> 1, k7 on a haloed bf16 sequence: |got - ref| <= (7 C + 1) 2^-24 sum |x w|; block edges 255 / 256 / 257 and the real 120000."""
    worst, failed = 0.0, []
    for C, L in E.CONV_OUT1:
        c = E.ConvOut1Case(C, L)
        x, w, out = _bf16(c.x_alloc), _f32(c.w), _f32(c.out_alloc())
        rc = lib.ezvae_conv_out1(x.data_ptr() + c.x0 * 2, c.ldx, w.data_ptr(), out.data_ptr() + E.VGUARD * 4, L, C, None)
        assert rc == 0, lib.ezdit_last_error()
        torch.cuda.synchronize()
        ex = c.excess(out.cpu().numpy())
        print(f'conv_out1 C{C} L{L}: excess {ex:.3e}')
        worst = max(worst, ex)
        if not ex <= 1.0:
            failed.append((C, L, ex))
    record(f'vae conv_out1: worst error / bound {worst:.3e}')
    assert not failed, failed


def test_vae_conv_in1_against_fp64(lib, dev):
    """1 -> C, k7 on a waveform between NaN guards (zero padding by index): |got - ref| <= 8 x 2^-24 (|b| + sum |x w|); T below, at and above the 7 taps."""
    worst, failed = 0.0, []
    for C, T in E.CONV_IN1:
        c = E.ConvIn1Case(C, T)
        wav, w, b, out = _f32(c.wav_alloc), _f32(c.w), _f32(c.b), _f32(c.out_alloc())
        rc = lib.ezvae_conv_in1(wav.data_ptr() + E.VGUARD * 4, w.data_ptr(), b.data_ptr(), out.data_ptr() + E.GUARD * C * 4, T, C, None)
        assert rc == 0, lib.ezdit_last_error()
        torch.cuda.synchronize()
        ex = c.excess(out.cpu().numpy())
        print(f'conv_in1 C{C} T{T}: excess {ex:.3e}')
        worst = max(worst, ex)
        if not ex <= 1.0:
            failed.append((C, T, ex))
    record(f'vae conv_in1: worst error / bound {worst:.3e}')
    assert not failed, failed


@pytest.mark.parametrize('with_noise', [True, False])
def test_vae_sample_against_fp64(lib, dev, with_noise):
    """L != latent, scale from where expf underflows to where it overflows (the threshold branch must win), noise present and NULL: rtol = atol = 1e-5 of
    float64 noise (logaddexp(0, scale) + 1e-4) + mean."""
    worst, failed = 0.0, []
    for lat, L in E.SAMPLE_SHAPES:
        c = E.SampleCase(lat, L, with_noise)
        enc, out = _f32(c.enc_alloc), _f32(c.out_alloc())
        noise = _f32(c.noise) if with_noise else None
        rc = lib.ezvae_sample(enc.data_ptr() + c.enc0 * 4, None if noise is None else noise.data_ptr(), out.data_ptr() + E.VGUARD * 4, L, lat, None)
        assert rc == 0, lib.ezdit_last_error()
        torch.cuda.synchronize()
        ex = c.excess(out.cpu().numpy())
        print(f'sample lat {lat} L{L} noise {with_noise}: excess {ex:.3e}')
        worst = max(worst, ex)
        if not ex <= 1.0:
            failed.append((lat, L, ex))
    record(f'vae sample noise {with_noise}: worst error / tolerance {worst:.3e}')
    assert not failed, failed
