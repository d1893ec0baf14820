"""CPU tests of the host side of the DPM-Solver++(2M) multistep solver: the coefficient c_hist against its formula in fp64, the solver's order
on a Gaussian toy whose probability-flow solution is known in closed form, the C ABI's declarations and the refusals that need no GPU, and the
`solver` keyword's validation in inference / generate_audio."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from ezaudio_amd.sampler import LatentSampler as _RealSampler    # (bound at collection: an earlier test module replaces the module attribute for good)
from tests.test_ragged_host import PARAMS, PROMPTS, _Tok, _Unet, _enc, _vae
from tests.util import DIFF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scheduler(K):
    from ezaudio_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(K)
    return sch


# ---------------------------------------------------------------------------------------------------
# 1. coefficients
# ---------------------------------------------------------------------------------------------------
def _c_hist_fp64(sch):
    """c_hist_i = alpha' (1 - e^{-h_i}) / (2 r_i), h_i = lambda' - lambda_i, r_i = h_{i-1} / h_i, lambda = ln(alpha / sigma); 0 where h_i or h_{i-1} is
    not finite.  Restated from alphas_cumprod alone: prev_t = t - 1000 // K, alpha_bar = 1 past the end."""
    ac = [float(v) for v in sch.alphas_cumprod]
    K = len(sch.timesteps)

    def lam(a):
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        if alpha == 0.0:
            return -math.inf
        if sigma == 0.0:
            return math.inf
        return math.log(alpha / sigma)
    hs, out = [], []
    for i, t in enumerate(int(t) for t in sch.timesteps):
        tp = t - 1000 // K
        ap = ac[tp] if tp >= 0 else 1.0
        hs.append(lam(ap) - lam(ac[t]))
        if i == 0 or not math.isfinite(hs[i]) or not math.isfinite(hs[i - 1]):
            out.append(0.0)
        else:
            out.append(math.sqrt(ap) * (1.0 - math.exp(-hs[i])) / (2.0 * (hs[i - 1] / hs[i])))
    return out


@pytest.mark.parametrize('K', [10, 25, 50])
def test_multistep_coefficients_are_the_formula_in_fp64(K):
    sch = _scheduler(K)
    got, want = sch.multistep_coefficients(), _c_hist_fp64(sch)
    assert len(got) == K and all(isinstance(v, float) for v in got)
    assert got[0] == 0.0 and got[1] == 0.0 and got[K - 1] == 0.0       # lambda = -inf at t = 999, +inf past the end: first-order steps
    for i in range(2, K - 1):
        assert math.isfinite(got[i]) and got[i] > 0.0, (i, got[i])
        assert abs(got[i] - want[i]) <= 1e-6 * abs(want[i]), (i, got[i], want[i])


# ---------------------------------------------------------------------------------------------------
# 2. the solver on a Gaussian toy: data x0 ~ N(0, s^2) per element, posterior-mean denoiser x0hat = alpha s^2 x / (alpha^2 s^2 + sigma^2);
#    the exact probability-flow solution from x_T is s x_T
# ---------------------------------------------------------------------------------------------------
def _toy(K, s2, multistep, zero_hist=False):
    sch = _scheduler(K)
    coefs = sch.ddim_coefficients(0)
    ch = sch.multistep_coefficients() if multistep else [0.0] * K
    if zero_hist:
        ch = [0.0] * K
    x, hist = 1.0, float('nan')
    for (sa, sb, cx0, cdir, sigma), c in zip(coefs, ch):
        assert sigma == 0.0
        x0hat = sa * s2 * x / (sa * sa * s2 + sb * sb)
        v = sa * ((x - sa * x0hat) / sb) - sb * x0hat      # the v-prediction of that denoiser (sb > 0 on every step's t)
        x0 = sa * x - sb * v
        eps = sa * v + sb * x
        nxt = cx0 * x0 + cdir * eps
        if multistep and c != 0.0:
            nxt += c * (x0 - hist)
        hist = x0
        x = nxt
    return x


@pytest.mark.parametrize('s2', [0.25, 1.0, 4.0])
def test_2m_beats_ddim_on_the_gaussian_toy(s2):
    s = math.sqrt(s2)
    for K in (10, 25, 50):
        e_ddim, e_2m, e_ddim2 = abs(_toy(K, s2, False) - s), abs(_toy(K, s2, True) - s), abs(_toy(2 * K, s2, False) - s)
        print(f'toy s2={s2} K={K}: DDIM {e_ddim:.3e}  2M {e_2m:.3e}  DDIM(2K) {e_ddim2:.3e}')
        assert math.isfinite(e_2m) and e_2m < e_ddim, (K, e_2m, e_ddim)
        if s2 >= 1.0:
            assert e_2m < e_ddim2, (K, e_2m, e_ddim2)
        assert _toy(K, s2, True, zero_hist=True) == _toy(K, s2, False)      # every c_hist 0: the DDIM run, exactly


# ---------------------------------------------------------------------------------------------------
# 3. ABI
# ---------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_binding_binds_the_multistep_entry_points(lib):
    from ezaudio_amd import _lib
    from oracle.weights import model_config
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ezdit.h')).read(), flags=re.S)
    for name, nargs in (('ezdit_sampler_set_multistep', 5), ('ezdit_cfg_multistep_step', 10)):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m and len(m.group(1).split(',')) == nargs, name
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib, name).argtypes == args
    assert '#define EZDIT_ABI_VERSION 4' in hdr and lib.ezdit_abi_version() == 4 and _lib.ABI_VERSION == 4    # additive: the version stays
    cfg = model_config('xs')
    c = _lib.EzditConfig(cfg['embed_dim'], cfg['num_heads'], cfg['depth'], cfg['in_chans'], cfg['out_chans'], cfg['context_dim'],
                         cfg['ada_sola_rank'], float(cfg['ada_sola_alpha']), float(cfg['mlp_ratio']), 2048)
    h = C.c_void_p()
    assert lib.ezdit_create(C.byref(c), C.byref(h)) == 0
    try:
        ch = (C.c_float * 4)(0.0, 0.0, 0.1, 0.0)
        assert lib.ezdit_sampler_set_multistep(h, ch, 4, None, None) == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_set_multistep(h, None, 0, None, None) == -3
        assert lib.ezdit_sampler_set_multistep(None, ch, 4, None, None) == -1
        assert lib.ezdit_set_step(h, 2, None) == -3                                  # (unchanged: no workspace)
    finally:
        lib.ezdit_destroy(h)
    assert lib.ezdit_cfg_multistep_step(None, None, None, None, None, 0, 1, 128, None, None) == -1


# ---------------------------------------------------------------------------------------------------
# 4. the `solver` keyword
# ---------------------------------------------------------------------------------------------------
class _RecordingSampler:
    seen = []

    def __init__(self, unet, scheduler):
        pass

    def prepare(self, text, text_mask, uncond, uncond_mask, init, step_noises, gs, gr, steps, eta, **kw):
        _RecordingSampler.seen.append(dict(eta=eta, noise=step_noises, kw=kw))
        self.lat = init

    def run(self, use_graph=True):
        pass

    def finish(self):
        return self.lat


def _infer(prompts, **kw):
    from ezaudio_amd import sampler as S
    args = dict(audio_frames=8, guidance_scale=5, guidance_rescale=0.0, ddim_steps=3, eta=1, random_seed=11)
    args.update(kw)
    return S.inference(_vae, _Unet(), None, None, _Tok(), _enc, PARAMS, None, prompts, None, device='cpu', **args)


def _ez():
    from ezaudio_amd import api
    ez = api.EzAudio.__new__(api.EzAudio)
    ez.device = 'cpu'
    ez.autoencoder, ez.unet, ez.tokenizer, ez.text_encoder, ez.noise_scheduler, ez.params = _vae, _Unet(), _Tok(), _enc, None, PARAMS
    return ez


def test_solver_keyword_is_validated_and_passed_through(monkeypatch):
    import inspect
    from ezaudio_amd import api, sampler as S
    _RecordingSampler.seen.clear()
    ez = _ez()
    for fn in (_RealSampler.prepare, S.inference, S.inference_controlnet, api.EzAudio.generate_audio, api.EzAudio.editing_audio,
               api.EzAudio_ControlNet.generate_audio):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == 'solver' and last.default == 'ddim', fn           # a new LAST keyword, default unchanged behaviour
    monkeypatch.setattr(S, 'LatentSampler', _RecordingSampler)
    n = 0
    for bad, word in ((dict(solver='heun'), 'solver'), (dict(solver='dpmpp_2m', eta=1), 'eta=0'), (dict(solver='dpmpp_2m'), 'eta=0'),
                      (dict(solver='dpmpp_2m', eta=[0, 1]), 'eta=0')):
        with pytest.raises(ValueError, match=word):
            _infer(PROMPTS[:2], **bad)
        with pytest.raises(ValueError, match=word):
            ez.generate_audio(PROMPTS[:2], length=1, ddim_steps=3, random_seed=3, **bad)
        assert len(_RecordingSampler.seen) == n                                # refused before anything was sampled
    with pytest.raises(ValueError, match='deterministic'):
        _infer(PROMPTS[:1], solver='dpmpp_2m', eta=0.5)
    # 'ddim' (given or defaulted) reaches the sampler as the call it has always been: no solver argument, nothing multistep
    _infer(PROMPTS[:2], solver='ddim')
    ez.generate_audio(PROMPTS[:2], length=1, ddim_steps=3, random_seed=3)
    assert len(_RecordingSampler.seen) == 2 and all(s['kw'].get('solver', 'ddim') == 'ddim' for s in _RecordingSampler.seen)
    # 'dpmpp_2m' with eta 0 (scalar or list of zeros) goes through, draws no step noise
    _infer(PROMPTS[:2], solver='dpmpp_2m', eta=0)
    ez.generate_audio(PROMPTS[:2], length=1, ddim_steps=3, random_seed=3, eta=[0, 0.0], solver='dpmpp_2m')
    for s in _RecordingSampler.seen[2:]:
        assert s['kw']['solver'] == 'dpmpp_2m' and s['noise'] is None
    assert len(_RecordingSampler.seen) == 4


def test_check_solver_and_prepare_refuse_before_touching_the_device():
    from ezaudio_amd.sampler import check_solver
    check_solver('ddim', 1)
    check_solver('dpmpp_2m', 0)
    check_solver('dpmpp_2m', None)
    check_solver('dpmpp_2m', [0, 0.0, None])
    check_solver('dpmpp_2m', torch.zeros(3))
    smp = _RealSampler.__new__(_RealSampler)                                   # no device: prepare must refuse first
    init = torch.zeros(2, 4, 8)
    for kw, word in ((dict(solver='euler', eta=0), 'solver'), (dict(solver='dpmpp_2m', eta=1), 'eta=0'),
                     (dict(solver='dpmpp_2m', eta=[0, 1]), 'eta=0')):
        with pytest.raises(ValueError, match=word):
            smp.prepare(None, None, None, None, init, None, 5.0, 0.0, 10, kw['eta'], solver=kw['solver'])
